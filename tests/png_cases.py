"""The pictures the PNG tests encode, shared by the numpy restatement's tests and the device's: float inputs of
mp_picture_png, each the smallest at which one mechanism of the definition (include/monoport_hip.h) can go wrong."""
import collections

import numpy as np

import png_ref as ref

F = np.float32
Case = collections.namedtuple("Case", ["name", "format", "image", "alpha", "unmatte", "lo", "scale"])


def case(name, fmt, image, alpha=None, unmatte=None, lo=0.0, scale=1.0):
    return Case(name, fmt, np.ascontiguousarray(image, F), None if alpha is None else np.ascontiguousarray(alpha, F),
                unmatte, lo, scale)


def noise(fmt, h, w, seed):
    """Uniform noise in every byte of the samples."""
    rng = np.random.RandomState(seed)
    if fmt == "gray16":
        return case("noise_%dx%d" % (h, w), fmt, rng.randint(0, 65536, (h, w)) / 65535.0)
    image = rng.randint(0, 256, (h, w, 3)) / 255.0
    return case("noise_%dx%d" % (h, w), fmt, image, rng.randint(0, 256, (h, w)) / 255.0 if fmt == "rgba8" else None)


def bytes_picture(name, values, w):
    """An RGB8 picture of one row whose samples are ``values`` (3 w of them in 0..255)."""
    return case(name, "rgb8", (np.asarray(values, np.float64) / 255.0).reshape(1, w, 3))


def no_match():
    """No byte of the stream equals the one 1, 3 or 6 before it, so no block has a match: the distance code of length
    zero."""
    return bytes_picture("no_match", (np.arange(1, 1 + 3 * 40) * 37) % 256, 40)


def fibonacci():
    """One block (filter None) whose literal counts obey the Fibonacci recurrence -- 1, 1 (the filter byte and the end
    of block), 1, 3, 4, 7, 11, ... (each count one more than all the smaller trees joined, which is what a chain needs
    under the definition's tie order; the plain Fibonacci numbers would need 4180 tokens for 17 leaves) -- with the last
    count raised to fill whole pixels: 17 leaves, an unlimited Huffman tree 16 deep.  The bytes are laid out so that
    every third one differs from those 1, 3 and 6 before it: no match takes a literal away."""
    counts = [1, 3, 4, 7, 11, 18, 29, 47, 76, 123, 199, 322, 521, 843, 1366]
    left = {13 * (i + 1): c for i, c in enumerate(counts)}
    n = sum(counts)
    x = [0]  # the filter byte
    for j in range(1, n + 1):
        order = sorted(left, key=lambda s: (-left[s], s))
        if j % 3 == 0:
            order = [s for s in order if s not in (x[j - 1], x[j - 3], x[j - 6] if j >= 6 else -1)]
        s = next(s for s in order if left[s] > 0)
        left[s] -= 1
        x.append(s)
    return bytes_picture("fibonacci", x[1:], n // 3)


# (width of one row of noise, pixels of it made constant at its end) whose RGB8 zlib streams under filter None are
# IDAT - 1, IDAT and IDAT + 1 bytes long: found by search, asserted by the restatement's test
IDAT_EDGE = {-1: (2703, 0), 0: (2702, 2), 1: (2733, 37)}


def idat_edge(delta):
    w, flat = IDAT_EDGE[delta]
    c = noise("rgb8", 1, w, 11)
    image = c.image.copy()
    image[:, w - flat:] = F(0.5)
    return c._replace(name="idat_%+d" % delta, image=image)


def special_values(fmt):
    """NaN, the infinities and values outside [0, 1] in the image, the alpha and the depth; alpha 0 with unmatte; a
    depth range one float wide."""
    odd = np.asarray([np.nan, np.inf, -np.inf, -1.0, 2.0, 0.0, -0.0, 1.0, 0.5, 1e-30, 0.999999, 254.5 / 255], F)
    rng = np.random.RandomState(3)
    if fmt == "gray16":
        d = rng.uniform(0.9, 1.1, (8, 9)).astype(F)
        d.reshape(-1)[:len(odd)] = odd
        d[3] = [np.nextafter(F(1), F(2))] * 4 + [1.0] * 5
        hi = np.nextafter(F(1), F(2))
        return case("special", fmt, d, lo=1.0, scale=float(F(1) / (hi - F(1))))
    image = rng.uniform(-0.2, 1.2, (8, 9, 3)).astype(F)
    image.reshape(-1)[:len(odd)] = odd
    if fmt == "rgb8":
        return case("special", fmt, image)
    alpha = rng.uniform(-0.2, 1.2, (8, 9)).astype(F)
    alpha.reshape(-1)[5:5 + len(odd)] = odd
    alpha[7] = [0.0, 1e-6, 0.25, 1.0, 0.0, 0.5, 0.75, 1e-3, 0.0]
    return case("special_unmatte", fmt, image, alpha, unmatte=0.75)


def smooth(fmt, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 0.5 + 0.45 * np.sin(yy / 9.0 + xx / 13.0)
    if fmt == "gray16":
        return case("smooth_%dx%d" % (h, w), fmt, v)
    image = np.stack([v, 0.5 + 0.45 * np.cos(xx / 7.0), 0.5 + 0.4 * np.sin(yy / 5.0)], -1)
    return case("smooth_%dx%d" % (h, w), fmt, image, np.clip(1.2 - v, 0, 1) if fmt == "rgba8" else None)


def constant(fmt, h, w):
    if fmt == "gray16":
        return case("constant_%dx%d" % (h, w), fmt, np.full((h, w), 0.3))
    return case("constant_%dx%d" % (h, w), fmt, np.full((h, w, 3), 0.3), np.full((h, w), 0.6) if fmt == "rgba8" else None)


# widths whose scanline stride 1 + w bpp lies just below, on (where it can) and above the 4096-byte block
EDGE_WIDTHS = {"rgb8": (1364, 1365, 1366), "rgba8": (1023, 1024), "gray16": (2047, 2048)}


def small_cases(fmt):
    """The cases of one format, a few kilobytes each."""
    out = [noise(fmt, 1, 1, 0), noise(fmt, 1, 37, 1), noise(fmt, 29, 1, 2), constant(fmt, 20, 300), constant(fmt, 1, 2000),
           noise(fmt, 64, 64, 4),
           smooth(fmt, 61, 83), special_values(fmt)]
    out += [smooth(fmt, 3, w)._replace(name="edge_%d" % w) for w in EDGE_WIDTHS[fmt]]
    if fmt == "rgb8":
        out += [no_match(), fibonacci()] + [idat_edge(d) for d in sorted(IDAT_EDGE)]
    if fmt == "rgba8":
        big = smooth(fmt, 16, 4096)
        rough = big.image + np.random.RandomState(6).uniform(-0.02, 0.02, big.image.shape)
        out.append(big._replace(name="wide_16x4096", image=np.ascontiguousarray(rough, F)))
    return out


def samples(c):
    return ref.samples_of(c.image, c.format, c.alpha, c.unmatte, c.lo, c.scale)


def restated(c, filter="adaptive"):
    """The restatement's file of a case."""
    return ref.encode(c.image, c.format, filter, c.alpha, c.unmatte, c.lo, c.scale)[0]
