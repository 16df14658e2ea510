"""The numpy restatement of mp_picture_u8 / mp_picture_jpeg (include/monoport_hip.h): baseline JFIF with restart
intervals, all-integer after the 8-bit step, and a small entropy decoder of our own streams back to the quantised
coefficients.  numpy only; the tables are literals (tests/golden/jpeg_tables.npz holds the same data)."""
import numpy as np

SUBSAMPLINGS = ("444", "420")
HEADER_BYTES = 629
BLOCK_MAX_BITS = 1660

# zig-zag position -> natural index (row * 8 + column)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)

# ITU-T T.81 Annex K.1, in zig-zag order (as a DQT segment carries them)
BASE_LUMA = np.array([16, 11, 12, 14, 12, 10, 16, 14, 13, 14, 18, 17, 16, 19, 24, 40, 26, 24, 22, 22, 24, 49, 35, 37, 29,
                      40, 58, 51, 61, 60, 57, 51, 56, 55, 64, 72, 92, 78, 64, 68, 87, 69, 55, 56, 80, 109, 81, 87, 95, 98,
                      103, 104, 103, 62, 77, 113, 121, 112, 100, 120, 92, 101, 103, 99], dtype=np.int64)
BASE_CHROMA = np.array([17, 18, 18, 24, 21, 24, 47, 26, 26, 47, 99, 66, 56, 66] + [99] * 50, dtype=np.int64)

# ITU-T T.81 Annex K.3: (codes per length 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193,
            21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56,
            57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106,
            115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151,
            152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194,
            195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229,
            230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9,
              35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54,
              55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104,
              105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
              149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184,
              185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227,
              228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])
# DHT order in the file: (class << 4 | selector, table)
HUFFMAN = ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA))

# C[u][x] = rint(8192 a(u) cos((2x + 1) u pi / 16)), computed once in float64 (dct_matrix() is the formula)
DCT = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
                [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
                [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
                [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
                [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
                [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
                [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
                [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], dtype=np.int64)


def dct_matrix():
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(8, dtype=np.float64)[None, :]
    a = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5)
    return np.rint(8192.0 * a * np.cos((2.0 * x + 1.0) * u * np.pi / 16.0)).astype(np.int64)


def zigzag_order():
    """The zig-zag walk of an 8 x 8 block, built from its rule (ZIGZAG is the literal)."""
    out = []
    for s in range(15):
        cells = [(y, s - y) for y in range(8) if 0 <= s - y < 8]
        if s % 2 == 0:
            cells.reverse()
        out += [y * 8 + x for y, x in cells]
    return np.array(out, dtype=np.int64)


def quant_tables(quality):
    """(luma, chroma) in zig-zag order, scaled as the IJG library scales them."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def huffman_codes(table):
    """symbol -> (code, length), canonical (T.81 Annex C)."""
    counts, symbols = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            out[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def to_u8(x):
    """Step 1 (mp_picture_u8): float32 -> uint8; the multiply and the add are two f32 operations; NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        t = np.where(x > 0, np.where(x < 1, x, np.float32(1)), np.float32(0)).astype(np.float32)
        v = (t * np.float32(255)).astype(np.float32) + np.float32(0.5)
    return v.astype(np.float32).astype(np.int32).astype(np.uint8)


def geometry(h, w, subsampling, restart=None):
    """(mcu side, MCU columns, MCU rows, blocks per MCU, restart, intervals)."""
    assert subsampling in SUBSAMPLINGS
    m = 8 if subsampling == "444" else 16
    mw, mh = (w + m - 1) // m, (h + m - 1) // m
    r = mw if not restart else int(restart)
    assert 1 <= r <= 65535
    return m, mw, mh, 3 if subsampling == "444" else 6, r, (mw * mh + r - 1) // r


def max_bytes(h, w, subsampling, restart=None):
    """mp_jpeg_max_bytes: header + 208 bytes per block, doubled for stuffing, + one marker per interval."""
    _, mw, mh, bpm, _, ni = geometry(h, w, subsampling, restart)
    return HEADER_BYTES + 416 * (mw * mh * bpm) + 2 * ni


def fdct_quant(blocks, q_zz):
    """blocks [n,8,8] of samples 0..255 -> quantised coefficients [n,64] in zig-zag order (steps 5 and 6)."""
    p = blocks.astype(np.int64) - 128
    a = (np.einsum("ux,nyx->nyu", DCT, p) + 1024) >> 11
    f = (np.einsum("vy,nyu->nvu", DCT, a) + 16384) >> 15
    assert np.abs(a).max(initial=0) < 2 ** 31 and np.abs(f).max(initial=0) < 2 ** 31
    fz = f.reshape(-1, 64)[:, ZIGZAG]
    q = q_zz[None, :]
    return np.sign(fz) * ((np.abs(fz) + (q >> 1)) // q)


def coefficients(u8, quality, subsampling):
    """Steps 2-6: uint8 [H,W,3] -> (coefficients [blocks,64] in scan order, component index per block)."""
    h, w = u8.shape[:2]
    m, mw, mh, bpm, _, _ = geometry(h, w, subsampling)
    ys = np.minimum(np.arange(mh * m), h - 1)
    xs = np.minimum(np.arange(mw * m), w - 1)
    px = u8[ys][:, xs].astype(np.int64)
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    if subsampling == "420":
        cb, cr = [(c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2 for c in (cb, cr)]
    ql, qc = quant_tables(quality)

    def blocks_of(plane, q):
        hh, ww = plane.shape
        t = plane.reshape(hh // 8, 8, ww // 8, 8).transpose(0, 2, 1, 3)
        return fdct_quant(t.reshape(-1, 8, 8), q).reshape(hh // 8, ww // 8, 64)

    by, bcb, bcr = blocks_of(y, ql), blocks_of(cb, qc), blocks_of(cr, qc)
    out = np.zeros((mh, mw, bpm, 64), dtype=np.int64)
    if subsampling == "444":
        out[:, :, 0], out[:, :, 1], out[:, :, 2] = by, bcb, bcr
        comp = [0, 1, 2]
    else:
        for k in range(4):
            out[:, :, k] = by[(k >> 1)::2, (k & 1)::2]
        out[:, :, 4], out[:, :, 5] = bcb, bcr
        comp = [0, 0, 0, 0, 1, 2]
    return out.reshape(-1, 64), np.tile(np.array(comp), mh * mw)


def header(h, w, quality, subsampling, restart):
    ql, qc = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((ql, qc)):
        out += bytes([0xFF, 0xDB, 0x00, 0x43, i]) + bytes(int(v) for v in q)
    hv = 0x11 if subsampling == "444" else 0x22
    out += bytes([0xFF, 0xC0, 0x00, 0x11, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc, (counts, symbols) in HUFFMAN:
        n = 3 + 16 + len(symbols)
        out += bytes([0xFF, 0xC4, n >> 8, n & 255, tc]) + bytes(counts) + bytes(symbols)
    out += bytes([0xFF, 0xDD, 0x00, 0x04, restart >> 8, restart & 255])
    out += bytes([0xFF, 0xDA, 0x00, 0x0C, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])
    assert len(out) == HEADER_BYTES
    return bytes(out)


def _category(v):
    return int(abs(int(v))).bit_length()


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length

    def put_value(self, v, cat):
        self.put(v if v >= 0 else v - 1, cat)

    def to_bytes(self):
        pad = -self.n % 8
        acc, n = (self.acc << pad) | ((1 << pad) - 1), self.n + pad
        return acc.to_bytes(n // 8, "big") if n else b""


def encode_coefficients(coef, comp, h, w, quality, subsampling, restart=None):
    """Step 7 and the container: quantised coefficients in scan order -> (bytes, stats)."""
    _, _, _, bpm, r, ni = geometry(h, w, subsampling, restart)
    dc_t = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)]
    ac_t = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA)]
    stats = dict(zrl=0, stuffed=0, dc_category=0, ac_category=0, intervals=ni, no_eob=False, block_bits=0)
    out = bytearray(header(h, w, quality, subsampling, r))
    n_mcu = coef.shape[0] // bpm
    for k in range(ni):
        bits, pred = _Bits(), [0, 0, 0]
        for g in range(k * r * bpm, min((k + 1) * r, n_mcu) * bpm):
            c, t = int(comp[g]), int(comp[g] > 0)
            start = bits.n
            blk = [int(v) for v in coef[g]]
            d = blk[0] - pred[c]
            pred[c] = blk[0]
            cat = _category(d)
            stats["dc_category"] = max(stats["dc_category"], cat)
            bits.put(*dc_t[t][cat])
            bits.put_value(d, cat)
            run = 0
            for i in range(1, 64):
                v = blk[i]
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    bits.put(*ac_t[t][0xF0])
                    stats["zrl"] += 1
                    run -= 16
                cat = _category(v)
                stats["ac_category"] = max(stats["ac_category"], cat)
                bits.put(*ac_t[t][(run << 4) | cat])
                bits.put_value(v, cat)
                run = 0
            if blk[63] == 0:
                bits.put(*ac_t[t][0x00])
            else:
                stats["no_eob"] = True
            stats["block_bits"] = max(stats["block_bits"], bits.n - start)
        raw = bits.to_bytes()
        stats["stuffed"] += raw.count(b"\xff")
        out += raw.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + (k & 7)]) if k < ni - 1 else b"\xff\xd9"
    assert stats["block_bits"] <= BLOCK_MAX_BITS
    return bytes(out), stats


def encode(picture, quality=90, subsampling="420", restart=None):
    """uint8 or float [H,W,3] -> (bytes of the JFIF file, stats).  stats: zrl (ZRL symbols), stuffed (0x00 bytes
    inserted), dc_category / ac_category (the largest), intervals, no_eob (some block's coefficient 63 is non-zero)."""
    picture = np.asarray(picture)
    u8 = picture if picture.dtype == np.uint8 else to_u8(picture)
    assert u8.ndim == 3 and u8.shape[2] == 3 and 1 <= u8.shape[0] <= 4096 and 1 <= u8.shape[1] <= 4096
    coef, comp = coefficients(u8, quality, subsampling)
    return encode_coefficients(coef, comp, u8.shape[0], u8.shape[1], quality, subsampling, restart)


def decode(data):
    """The entropy decoder of our own streams: bytes -> (coefficients [blocks,64] in scan order, h, w, subsampling,
    restart).  It reads the geometry and the restart interval from the header and the Huffman tables from this file."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    i, h = 2, None
    while True:
        assert data[i] == 0xFF
        m, n = data[i + 1], (data[i + 2] << 8) | data[i + 3]
        seg = data[i + 4:i + 2 + n]
        if m == 0xC0:
            h, w = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4]
            subsampling = {0x11: "444", 0x22: "420"}[seg[7]]
        elif m == 0xDD:
            restart = (seg[0] << 8) | seg[1]
        i += 2 + n
        if m == 0xDA:
            break
    _, mw, mh, bpm, r, ni = geometry(h, w, subsampling, restart)
    comp = [0, 1, 2] if bpm == 3 else [0, 0, 0, 0, 1, 2]
    lookup = []
    for t in ((DC_LUMA, DC_CHROMA), (AC_LUMA, AC_CHROMA)):
        lookup.append([{(length, code): s for s, (code, length) in huffman_codes(x).items()} for x in t])
    body, coef, n_mcu = data[i:-2], [], mw * mh
    pos = 0
    for k in range(ni):
        end = pos
        while end < len(body) and not (body[end] == 0xFF and body[end + 1] != 0x00):
            end += 2 if body[end] == 0xFF else 1
        raw = body[pos:end].replace(b"\xff\x00", b"\xff")
        if k < ni - 1:
            assert body[end] == 0xFF and body[end + 1] == 0xD0 + (k & 7)
        pos = end + 2
        acc, nbits, at = int.from_bytes(raw, "big"), 8 * len(raw), 0

        def take(n):
            nonlocal at
            v = (acc >> (nbits - at - n)) & ((1 << n) - 1) if n else 0
            at += n
            return v

        def symbol(table):
            code = 0
            for length in range(1, 17):
                code = (code << 1) | take(1)
                if (length, code) in table:
                    return table[(length, code)]
            raise AssertionError("no Huffman code")

        def value(cat):
            v = take(cat)
            return v if cat == 0 or v >> (cat - 1) else v - (1 << cat) + 1

        pred = [0, 0, 0]
        for g in range(k * r * bpm, min((k + 1) * r, n_mcu) * bpm):
            c = comp[g % bpm]
            t = int(c > 0)
            blk = [0] * 64
            pred[c] += value(symbol(lookup[0][t]))
            blk[0] = pred[c]
            j = 1
            while j < 64:
                s = symbol(lookup[1][t])
                if s == 0x00:
                    break
                if s == 0xF0:
                    j += 16
                    continue
                j += s >> 4
                blk[j] = value(s & 15)
                j += 1
            coef.append(blk)
        rem = nbits - at
        assert rem < 8 and take(rem) == (1 << rem) - 1, "padding"
    assert pos == len(body) + 2
    return np.array(coef, dtype=np.int64), h, w, subsampling, restart
