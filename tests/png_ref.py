"""The numpy restatement of mp_picture_u16 / mp_picture_rgba8 / mp_picture_png (include/monoport_hip.h): PNG files in
8-bit RGB, 8-bit RGBA and 16-bit grey whose deflate stream is this library's own definition -- blocks of 4096 filtered
bytes, the longest match among at most seven fixed distances, a greedy parse per block, one dynamic-Huffman code per
block.  All-integer after the samples.  numpy, heapq and the two checksums of zlib only."""
import heapq
import struct
import zlib

import numpy as np

from jpeg_ref import to_u8

FORMATS = {"rgb8": (3, 8, 2), "rgba8": (4, 8, 6), "gray16": (2, 16, 0)}  # bytes per pixel, bit depth, colour type
FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")
BLOCK = 4096       # filtered bytes per deflate block, which is also the parse unit
IDAT = 8192        # data bytes per IDAT chunk (the last one shorter)
MAX_SIDE = 4096
SIGNATURE = b"\x89PNG\r\n\x1a\n"
MIN_BYTES = 8 + 25 + 12 + 12   # the smallest capacity the call accepts: signature, IHDR, an empty IDAT, IEND

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
            258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_CODE = np.zeros(259, np.int64)
for _c in range(29):
    LEN_CODE[LEN_BASE[_c]:] = _c
LEN_CODE[258] = 28


def to_u16(d, lo, scale):
    """GRAY16 samples (mp_picture_u16): t = (d - lo) * scale as two f32 operations, clamped to [0, 1] (a NaN: 0),
    (int)(t * 65535 + 0.5) with the multiply and the add separately rounded."""
    d = np.asarray(d, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((d - np.float32(lo)).astype(np.float32) * np.float32(scale)).astype(np.float32)
        t = np.where(t > 0, np.where(t < 1, t, np.float32(1)), np.float32(0)).astype(np.float32)
        v = (t * np.float32(65535)).astype(np.float32) + np.float32(0.5)
    return v.astype(np.float32).astype(np.int32).astype(np.uint16)


def to_rgba8(image, alpha, unmatte=None):
    """RGBA8 samples (mp_picture_rgba8): image [...,3] f32, alpha [...] f32 -> uint8 [...,4].  ``unmatte``: None, or the
    background value bg: for a > 0 the colour is (c - (1 - a) * bg) / a in four separately rounded f32 operations; for
    a <= 0 or a NaN, colour and alpha are 0."""
    c = np.asarray(image, dtype=np.float32)
    a = np.asarray(alpha, dtype=np.float32)
    assert c.shape[:-1] == a.shape and c.shape[-1] == 3
    out = np.empty(a.shape + (4,), np.uint8)
    out[..., 3] = to_u8(a)
    if unmatte is None:
        out[..., :3] = to_u8(c)
        return out
    with np.errstate(all="ignore"):
        seen = a > 0
        t = (np.float32(1) - a).astype(np.float32)
        t = (t * np.float32(unmatte)).astype(np.float32)[..., None]
        s = ((c - t).astype(np.float32) / a[..., None]).astype(np.float32)
    out[..., :3] = np.where(seen[..., None], to_u8(s), 0)
    out[..., 3] = np.where(seen, out[..., 3], 0)
    return out


def format_of(samples):
    s = np.asarray(samples)
    if s.dtype == np.uint16 and s.ndim == 2:
        return "gray16"
    assert s.dtype == np.uint8 and s.ndim == 3 and s.shape[2] in (3, 4), (s.dtype, s.shape)
    return "rgb8" if s.shape[2] == 3 else "rgba8"


def rows_of(samples):
    """The unfiltered scanlines [H, W * bpp] uint8 (16-bit samples big-endian) and bpp."""
    fmt = format_of(samples)
    s = np.asarray(samples)
    if fmt == "gray16":
        s = np.stack([s >> 8, s & 255], axis=-1).astype(np.uint8)
    return np.ascontiguousarray(s.reshape(s.shape[0], -1)), FORMATS[fmt][0]


def filtered_stream(samples, filter="adaptive"):
    """The bytes deflate sees: per scanline the filter type and the filtered bytes.  ``adaptive``: the type with the
    smallest sum of |signed byte| over the line, ties to the lowest type."""
    assert filter in FILTERS
    raw, bpp = rows_of(samples)
    h, n = raw.shape
    x = raw.astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp] if n > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp] if n > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    f = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255       # [5,H,n]
    if filter == "adaptive":
        cost = np.where(f < 128, f, 256 - f).sum(axis=2)                      # [5,H]
        kind = np.argmin(cost, axis=0)                                        # the first of equal minima
    else:
        kind = np.full(h, FILTERS.index(filter))
    out = np.empty((h, n + 1), np.uint8)
    out[:, 0] = kind
    out[:, 1:] = f[kind, np.arange(h)]
    return out.reshape(-1)


def unfilter(stream, h, w, bpp):
    """The scanlines [H, W * bpp] of a filtered stream (the PNG specification's reconstruction)."""
    s = np.frombuffer(bytes(stream), np.uint8).reshape(h, 1 + w * bpp)
    out = np.zeros((h, w * bpp), np.int64)
    for y in range(h):
        kind = int(s[y, 0])
        assert kind < 5
        up = out[y - 1] if y else np.zeros(w * bpp, np.int64)
        for i in range(w * bpp):
            a = out[y, i - bpp] if i >= bpp else 0
            b = up[i]
            c = up[i - bpp] if i >= bpp else 0
            if kind == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            else:
                pred = (0, a, b, (a + b) >> 1)[kind]
            out[y, i] = (int(s[y, 1 + i]) + pred) & 255
    return out.astype(np.uint8)


def candidates(w, bpp):
    """The distances a match may have, ascending: 1, a pixel, two pixels, the scanline stride and the pixels left and
    right of it, two strides -- those of them in 1..32768."""
    stride = 1 + w * bpp
    return sorted(d for d in {1, bpp, 2 * bpp, stride - bpp, stride, stride + bpp, 2 * stride} if 1 <= d <= 32768)


def matches(x, cands):
    """Per position the longest match (0: none) and its distance: per candidate the run of x[j] == x[j - d] from the
    position on, not past the block's end, at most 258; a longer run wins, the smaller distance on a tie."""
    n = len(x)
    idx = np.arange(n)
    end = np.minimum((idx // BLOCK + 1) * BLOCK, n)
    best = np.zeros(n, np.int64)
    dist = np.zeros(n, np.int64)
    for d in cands:
        eq = np.zeros(n, bool)
        if d < n:
            eq[d:] = x[d:] == x[:-d]
        miss = np.minimum.accumulate(np.where(eq, n, idx)[::-1])[::-1]
        run = np.minimum(np.minimum(miss, end) - idx, 258)
        better = (run > best) & (run >= 3)
        best[better] = run[better]
        dist[better] = d
    return best, dist


def huffman_lengths(counts, limit):
    """Code lengths of the symbols with a non-zero count.  No such symbol: all 0; one: length 1.  Else a Huffman tree:
    the live node with the smallest (weight, index) and then the next one are joined into a node whose index follows
    every earlier one (leaves are their symbols; so a leaf goes before a joined node, a lower symbol and an earlier
    join first).  A tree deeper than ``limit``: every non-zero count becomes (c + 1) >> 1 and the tree is built again."""
    counts = [int(c) for c in counts]
    n = len(counts)
    while True:
        used = [s for s in range(n) if counts[s] > 0]
        lens = [0] * n
        if len(used) < 2:
            for s in used:
                lens[s] = 1
            return lens
        heap = [(counts[s], s) for s in used]
        heapq.heapify(heap)
        parent = {}
        m = 0
        while len(heap) > 1:
            wa, ia = heapq.heappop(heap)
            wb, ib = heapq.heappop(heap)
            parent[ia] = parent[ib] = n + m
            heapq.heappush(heap, (wa + wb, n + m))
            m += 1
        root = n + m - 1
        for s in used:
            p = s
            while p != root:
                p = parent[p]
                lens[s] += 1
        if max(lens) <= limit:
            return lens
        counts = [(c + 1) >> 1 if c > 0 else 0 for c in counts]


def canonical(lens):
    """RFC 1951 3.2.2: the codes of these lengths, bit-reversed (as they go into the LSB-first stream)."""
    top = max(max(lens), 1)
    count = [0] * (top + 1)
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt = [0] * (top + 2)
    code = 0
    for bits in range(1, top + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for v in lens:
        if v == 0:
            out.append(0)
            continue
        c = nxt[v]
        nxt[v] += 1
        out.append(int(format(c, "0%db" % v)[::-1], 2))
    return out


def run_lengths(seq):
    """The code-length sequence as (symbol, extra bits, extra value): a run of zeros is taken from its start as 18
    (11..138) while at least 11 remain, then 17 (3..10), then single zeros; a run of a length v as v, then 16 (3..6)
    while at least 3 remain, then single v."""
    out = []
    i = 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r > 0:
                if r >= 11:
                    k = min(r, 138)
                    out.append((18, 7, k - 11))
                elif r >= 3:
                    k = r
                    out.append((17, 3, k - 3))
                else:
                    k = 1
                    out.append((0, 0, 0))
                r -= k
        else:
            out.append((v, 0, 0))
            r -= 1
            while r >= 3:
                k = min(r, 6)
                out.append((16, 2, k - 3))
                r -= k
            out.extend([(v, 0, 0)] * r)
    return out


def dist_symbol(d):
    s = max(i for i in range(30) if DIST_BASE[i] <= d)
    return s, DIST_EXTRA[s], d - DIST_BASE[s]


def put_bits(vals, nbits):
    """(value, bit count) pairs -> the bits, each value LSB first."""
    vals = np.asarray(vals, dtype=np.uint64)
    nbits = np.asarray(nbits, dtype=np.int64)
    off = np.cumsum(nbits) - nbits
    bits = np.zeros(int(nbits.sum()), np.uint8)
    for b in range(int(nbits.max(initial=0))):
        m = nbits > b
        bits[off[m] + b] = (vals[m] >> np.uint64(b)) & np.uint64(1)
    return bits


def block_tokens(x, lo, hi, best, dist):
    """The greedy parse of x[lo:hi]: (token starts, match lengths (< 3: a literal), distances, literal/length symbols,
    {distance: (symbol, extra bits, extra value)}, the two histograms, the end-of-block symbol counted)."""
    starts = []
    i = lo
    while i < hi:
        starts.append(i)
        i += int(best[i]) if best[i] >= 3 else 1
    starts = np.asarray(starts)
    mlen, mdist = best[starts], dist[starts]
    is_m = mlen >= 3
    lsym = np.where(is_m, 257 + LEN_CODE[np.where(is_m, mlen, 3)], x[starts])
    ll_hist = np.bincount(lsym, minlength=286)
    ll_hist[256] += 1
    dinfo = {int(d): dist_symbol(int(d)) for d in np.unique(mdist[is_m])}
    d_hist = np.zeros(30, np.int64)
    for d in mdist[is_m]:
        d_hist[dinfo[int(d)][0]] += 1
    return starts, mlen, mdist, lsym, dinfo, ll_hist, d_hist


def block_bits(x, lo, hi, best, dist, final):
    """The bits of the dynamic-Huffman block of x[lo:hi]."""
    starts, mlen, mdist, lsym, dinfo, ll_hist, d_hist = block_tokens(x, lo, hi, best, dist)
    is_m = mlen >= 3
    ll_len = huffman_lengths(ll_hist, 15)
    d_len = huffman_lengths(d_hist, 15)
    hlit = max(257, max(s for s in range(286) if ll_len[s]) + 1)
    hdist = max([1] + [s + 1 for s in range(30) if d_len[s]])
    tokens = run_lengths(ll_len[:hlit] + d_len[:hdist])
    cl_hist = np.bincount([t[0] for t in tokens], minlength=19)
    cl_len = huffman_lengths(cl_hist, 7)
    hclen = max(4, max(i for i in range(19) if cl_len[CL_ORDER[i]]) + 1)
    ll_code, d_code, cl_code = canonical(ll_len), canonical(d_len), canonical(cl_len)
    vals = [1 if final else 0, 2, hlit - 257, hdist - 1, hclen - 4]
    nbits = [1, 2, 5, 5, 4]
    for i in range(hclen):
        vals.append(cl_len[CL_ORDER[i]])
        nbits.append(3)
    for sym, eb, ev in tokens:
        vals.append(cl_code[sym] | (ev << cl_len[sym]))
        nbits.append(cl_len[sym] + eb)
    ll_code, ll_len_a = np.asarray(ll_code, np.int64), np.asarray(ll_len, np.int64)
    v = ll_code[lsym]
    nb = ll_len_a[lsym]
    if is_m.any():
        lc = LEN_CODE[np.where(is_m, mlen, 3)]
        lextra = np.asarray(LEN_EXTRA)[lc]
        lval = np.where(is_m, mlen, 3) - np.asarray(LEN_BASE)[lc]
        dsym = np.asarray([dinfo[int(d)][0] if m else 0 for d, m in zip(mdist, is_m)])
        dextra = np.asarray([dinfo[int(d)][1] if m else 0 for d, m in zip(mdist, is_m)])
        dval = np.asarray([dinfo[int(d)][2] if m else 0 for d, m in zip(mdist, is_m)])
        dc, dl = np.asarray(d_code, np.int64)[dsym], np.asarray(d_len, np.int64)[dsym]
        mv = v | (lval << nb) | (dc << (nb + lextra)) | (dval << (nb + lextra + dl))
        v = np.where(is_m, mv, v)
        nb = np.where(is_m, nb + lextra + dl + dextra, nb)
    vals = np.concatenate([np.asarray(vals, np.int64), v, [ll_code[256]]])
    nbits = np.concatenate([np.asarray(nbits, np.int64), nb, [ll_len_a[256]]])
    return put_bits(vals, nbits)


def deflate(x, w, bpp):
    """The zlib stream of the filtered bytes x: 0x78 0x01, the blocks back to back, zero bits to a byte, Adler-32."""
    x = np.frombuffer(bytes(x), np.uint8).astype(np.int64)
    best, dist = matches(x, candidates(w, bpp))
    nblk = (len(x) + BLOCK - 1) // BLOCK
    bits = [block_bits(x, k * BLOCK, min((k + 1) * BLOCK, len(x)), best, dist, k == nblk - 1) for k in range(nblk)]
    body = np.packbits(np.concatenate(bits), bitorder="little").tobytes()
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(x.astype(np.uint8).tobytes()))


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode_samples(samples, filter="adaptive"):
    """The PNG file of uint8 [H,W,3] / [H,W,4] or uint16 [H,W] samples."""
    fmt = format_of(samples)
    h, w = np.asarray(samples).shape[:2]
    assert 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE
    bpp, depth, colour = FORMATS[fmt]
    z = deflate(filtered_stream(samples, filter), w, bpp)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 0))
    for i in range(0, len(z), IDAT):
        out += chunk(b"IDAT", z[i:i + IDAT])
    return out + chunk(b"IEND", b"")


def samples_of(image, format="rgb8", alpha=None, unmatte=None, lo=0.0, scale=1.0):
    if format == "rgb8":
        return to_u8(image)
    if format == "rgba8":
        return to_rgba8(image, alpha, unmatte)
    assert format == "gray16"
    return to_u16(image, lo, scale)


def encode(image, format="rgb8", filter="adaptive", alpha=None, unmatte=None, lo=0.0, scale=1.0):
    """mp_picture_png of one float picture -> (file, its size)."""
    f = encode_samples(samples_of(image, format, alpha, unmatte, lo, scale), filter)
    return f, len(f)


def max_bytes(h, w, format):
    """mp_png_max_bytes: a token covers at least one byte at 16 bits per byte at most (a literal: 15; a match of three
    bytes: 15 + 5 + 15 + 13), a block adds 3 + 14 + 19 * 3 + 316 * 7 + 15 = 2301 bits (288 bytes) of header and end."""
    s = h * (1 + w * FORMATS[format][0])
    z = 2 + 2 * s + 288 * ((s + BLOCK - 1) // BLOCK) + 4
    return 8 + 25 + 12 * ((z + IDAT - 1) // IDAT) + z + 12


def chunks_of(file):
    """[(type, data, crc)] of a PNG file, the signature checked."""
    assert file[:8] == SIGNATURE
    out, i = [], 8
    while i < len(file):
        n, = struct.unpack(">I", file[i:i + 4])
        out.append((file[i + 4:i + 8], file[i + 8:i + 8 + n], struct.unpack(">I", file[i + 8 + n:i + 12 + n])[0]))
        i += 12 + n
    assert i == len(file)
    return out
