"""The binary glTF file of mp_mesh_glb (include/monoport_hip.h) restated in numpy, byte for byte, and a minimal GLB
reader that follows the glTF 2.0 specification and KHR_mesh_quantization alone: it shares no code with the writer, so a
file that reads back within the quantisation steps is a file any viewer loads."""
import json
import struct

import numpy as np

F = np.float32
MIN_BYTES = 100  # MP_GLB_MIN_BYTES
ASSET = '{"asset":{"version":"2.0","generator":"monoport_amd"}'
EMPTY_JSON = ASSET + ',"scene":0,"scenes":[{}]}'


# ---- the writer: the definition, step by step -------------------------------------------------------------------------
def _truncated(x, where):
    """(int)x where ``where`` holds (there x is finite), else 0."""
    return np.where(where, np.trunc(np.where(where, x, F(0))), 0).astype(np.int64)


def quantise_positions(verts, b_min, b_max):
    """[n,3] f32 -> [n,3] ints in 0..65535: t = (x - b_min) * inv in two f32 operations, rounded half up, clamped."""
    b_min, b_max = np.asarray(b_min, F), np.asarray(b_max, F)
    inv = (F(65535.0) / (b_max - b_min)).astype(F)
    with np.errstate(all="ignore"):
        t = ((np.asarray(verts, F) - b_min).astype(F) * inv).astype(F)
        inside = (t > 0) & (t < F(65535.0))
        r = _truncated((t + F(0.5)).astype(F), inside)
    return np.where(t > 0, np.where(t < F(65535.0), r, 65535), 0).astype(np.int64)  # a NaN fails t > 0


def quantise_normals(normals):
    """[n,3] f32 -> [n,3] ints in -127..127."""
    n = np.asarray(normals, F)
    with np.errstate(all="ignore"):
        t = np.where(np.isnan(n), F(0), np.where(n > F(-1), np.where(n < F(1), n, F(1)), F(-1))).astype(F)
        m = (t * F(127.0)).astype(F)
        r = (m + np.where(t < 0, F(-0.5), F(0.5)).astype(F)).astype(F)
    return np.trunc(r).astype(np.int64)


def to_u8(c):
    """Step 1 of the JPEG definition (mp_picture_u8)."""
    c = np.asarray(c, F)
    with np.errstate(all="ignore"):
        t = np.where(c > 0, np.where(c < F(1), c, F(1)), F(0)).astype(F)
        return np.trunc(((t * F(255.0)).astype(F) + F(0.5)).astype(F)).astype(np.int64)


def quantise_colours(colours, scale=1.0, bias=0.0):
    """[n,3] f32 -> [n,3] ints in 0..255: c = p * scale + bias in two operations, then the 8-bit rule."""
    with np.errstate(all="ignore"):
        c = ((np.asarray(colours, F) * F(scale)).astype(F) + F(bias)).astype(F)
    return to_u8(c)


def _number(v, width):
    return ("%d" % v).rjust(width)


def json_text(flags, b_min, b_max, nv, nf, qmin, qmax, layout):
    """The JSON chunk's text (padded) of a non-empty mesh; ``layout``: the dict of ``bin_layout``."""
    nrm, col = flags
    k = 1 + nrm + col
    b_min, b_max = np.asarray(b_min, F).astype(np.float64), np.asarray(b_max, F).astype(np.float64)
    real = lambda x: "%24.17g" % x  # noqa: E731
    t = ASSET + ',"extensionsUsed":["KHR_mesh_quantization"],"extensionsRequired":["KHR_mesh_quantization"]'
    t += ',"scene":0,"scenes":[{"nodes":[0]}],"nodes":[{"mesh":0,"translation":['
    t += ",".join(real(b_min[a]) for a in range(3)) + '],"scale":['
    t += ",".join(real((b_max[a] - b_min[a]) / 65535.0) for a in range(3))
    t += ']}],"materials":[{"doubleSided":true}],"meshes":[{"primitives":[{"attributes":{"POSITION":0'
    if nrm:
        t += ',"NORMAL":1'
    if col:
        t += ',"COLOR_0":%d' % (k - 1)
    t += '},"indices":%d,"material":0,"mode":4}]}],"accessors":[' % k
    t += '{"bufferView":0,"componentType":5123,"count":%s,"type":"VEC3","min":[%s],"max":[%s]}' % (
        _number(nv, 10), ",".join(_number(v, 5) for v in qmin), ",".join(_number(v, 5) for v in qmax))
    if nrm:
        t += ',{"bufferView":1,"componentType":5120,"normalized":true,"count":%s,"type":"VEC3"}' % _number(nv, 10)
    if col:
        t += ',{"bufferView":%d,"componentType":5121,"normalized":true,"count":%s,"type":"VEC3"}' % (k - 1, _number(nv, 10))
    t += ',{"bufferView":%d,"componentType":%s,"count":%s,"type":"SCALAR"}],"bufferViews":[' % (
        k, _number(5125 if layout["wide"] else 5123, 4), _number(3 * nf, 10))
    view = '{"buffer":0,"byteOffset":%s,"byteLength":%s'
    t += view % (_number(0, 10), _number(8 * nv, 10)) + ',"byteStride":8,"target":34962}'
    if nrm:
        t += "," + view % (_number(layout["off_n"], 10), _number(4 * nv, 10)) + ',"byteStride":4,"target":34962}'
    if col:
        t += "," + view % (_number(layout["off_c"], 10), _number(4 * nv, 10)) + ',"byteStride":4,"target":34962}'
    t += "," + view % (_number(layout["off_i"], 10), _number(layout["idx_bytes"], 10)) + ',"target":34963}'
    t += '],"buffers":[{"byteLength":%s}]}' % _number(layout["bin"], 10)
    return t + " " * ((12 - len(t) % 8) % 8)  # to a length % 8 == 4: the binary data starts at a multiple of 8


def bin_layout(nv, nf, flags):
    nrm, col = flags
    wide = nv > 65535
    off_n = 8 * nv
    off_c = off_n + (4 * nv if nrm else 0)
    off_i = off_c + (4 * nv if col else 0)
    idx_bytes = (12 if wide else 6) * nf
    return dict(wide=wide, off_n=off_n, off_c=off_c, off_i=off_i, idx_bytes=idx_bytes,
                bin=(off_i + idx_bytes + 3) // 4 * 4)


def json_len(flags):
    """The padded text's length: a constant per attribute set."""
    z = (0, 0, 0)
    return len(json_text(flags, z, (1, 1, 1), 1, 1, z, z, bin_layout(1, 1, flags)))


def file_bytes(nv, nf, normals=True, colors=True):
    """mp_glb_bytes: the closed form of the file's size."""
    if nv == 0 or nf == 0:
        return MIN_BYTES
    flags = (bool(normals), bool(colors))
    return 12 + 8 + json_len(flags) + 8 + bin_layout(nv, nf, flags)["bin"]


def _chunk(kind, data):
    return struct.pack("<I4s", len(data), kind) + data


def encode(verts, faces, counts=None, normals=None, colors=None, color_layout="rows", color_scale=1.0, color_bias=0.0,
           b_min=(-1, -1, -1), b_max=(1, 1, 1)):
    """The file of the mesh in capacity-sized arrays verts [max_v,3] f32, faces [max_f,3] int32 under ``counts`` (None:
    all rows), with normals [max_v,3] and colours ([max_v,3] "rows" / [3,max_v] "planes") if given -> bytes."""
    verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    counts = (len(verts), len(faces)) if counts is None else counts
    nv = min(max(int(counts[0]), 0), len(verts))
    nf = min(max(int(counts[1]), 0), len(faces))
    if nv == 0 or nf == 0:
        text = EMPTY_JSON.encode("ascii")
        text += b" " * (-len(text) % 4)
        body = _chunk(b"JSON", text)
        return struct.pack("<4sII", b"glTF", 2, 12 + len(body)) + body
    flags = (normals is not None, colors is not None)
    layout = bin_layout(nv, nf, flags)
    q = quantise_positions(verts[:nv], b_min, b_max)
    pos = np.zeros((nv, 4), "<u2")
    pos[:, :3] = q
    data = pos.tobytes()
    if normals is not None:
        rows = np.zeros((nv, 4), np.uint8)
        rows[:, :3] = quantise_normals(np.asarray(normals, F).reshape(-1, 3)[:nv]) & 0xFF
        data += rows.tobytes()
    if colors is not None:
        c = np.asarray(colors, F)
        c = c.reshape(3, -1).T if color_layout == "planes" else c.reshape(-1, 3)
        rows = np.zeros((nv, 4), np.uint8)
        rows[:, :3] = quantise_colours(c[:nv], color_scale, color_bias)
        data += rows.tobytes()
    idx = np.clip(faces[:nf].astype(np.int64), 0, nv - 1).reshape(-1)
    data += idx.astype("<u4" if layout["wide"] else "<u2").tobytes()
    data += b"\0" * (-len(data) % 4)
    assert len(data) == layout["bin"]
    text = json_text(flags, b_min, b_max, nv, nf, q.min(axis=0), q.max(axis=0), layout).encode("ascii")
    body = _chunk(b"JSON", text) + _chunk(b"BIN\0", data)
    return struct.pack("<4sII", b"glTF", 2, 12 + len(body)) + body


# ---- the reader: the glTF 2.0 specification, nothing of the above -------------------------------------------------------
COMPONENTS = {5120: ("i1", 1), 5121: ("u1", 1), 5122: ("<i2", 2), 5123: ("<u2", 2), 5125: ("<u4", 4), 5126: ("<f4", 4)}
WIDTHS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4}


class Glb:
    """A parsed file: ``json`` (the document), ``chunks`` [(type, offset of the data in the file, data)], ``bin``."""

    def __init__(self, data):
        magic, version, total = struct.unpack_from("<4sII", data, 0)
        if magic != b"glTF" or version != 2:
            raise ValueError("not a glTF 2 binary file")
        if total != len(data):
            raise ValueError("the header says %d bytes, the file has %d" % (total, len(data)))
        self.chunks = []
        at = 12
        while at < total:
            size, kind = struct.unpack_from("<I4s", data, at)
            if size % 4 or at % 4:
                raise ValueError("a chunk of %d bytes at %d: not 4-byte aligned" % (size, at))
            self.chunks.append((kind, at + 8, data[at + 8:at + 8 + size]))
            at += 8 + size
        if at != total or not self.chunks or self.chunks[0][0] != b"JSON":
            raise ValueError("the chunks do not fill the file, or the first one is not JSON")
        self.json = json.loads(self.chunks[0][2].decode("utf-8"))
        self.bin = self.chunks[1][2] if len(self.chunks) > 1 else None
        if len(self.chunks) > 1 and self.chunks[1][0] != b"BIN\0":
            raise ValueError("the second chunk is not BIN")

    def accessor(self, index, raw=False):
        """The accessor's elements [count, width]: the stored integers with ``raw``, else as the specification (and for
        normalised integers its formulas) turns them into floats; integers stay integers where not normalised."""
        acc = self.json["accessors"][index]
        view = self.json["bufferViews"][acc["bufferView"]]
        if view["buffer"] != 0 or "uri" in self.json["buffers"][0]:
            raise ValueError("only the GLB-stored buffer is read")
        dtype, size = COMPONENTS[acc["componentType"]]
        width = WIDTHS[acc["type"]]
        stride = view.get("byteStride", size * width)
        start = view.get("byteOffset", 0) + acc.get("byteOffset", 0)
        if start % size or (("byteStride" in view) and stride % 4) or view.get("byteOffset", 0) % 4:
            raise ValueError("accessor %d is misaligned" % index)
        count = acc["count"]
        if count and start + stride * (count - 1) + size * width > view.get("byteOffset", 0) + view["byteLength"]:
            raise ValueError("accessor %d leaves its buffer view" % index)
        if view.get("byteOffset", 0) + view["byteLength"] > self.json["buffers"][0]["byteLength"] \
                or self.json["buffers"][0]["byteLength"] > len(self.bin):
            raise ValueError("a buffer view leaves the buffer")
        rows = np.empty((count, width), dtype)
        for j in range(width):
            rows[:, j] = np.ndarray((count,), dtype, self.bin, start + j * size, (stride,))
        if raw or not acc.get("normalized", False):
            return rows.astype(np.int64) if dtype != "<f4" else rows
        c = rows.astype(np.float64)
        return {"i1": np.maximum(c / 127.0, -1.0), "u1": c / 255.0, "<i2": np.maximum(c / 32767.0, -1.0),
                "<u2": c / 65535.0}[dtype]

    def mesh(self):
        """The one primitive of the one node of the scene: dict with ``positions`` [nv,3] float64 in world coordinates
        (the node's scale and translation applied), ``normals`` / ``colors`` or None, ``faces`` [nf,3]."""
        doc = self.json
        nodes = doc["scenes"][doc.get("scene", 0)].get("nodes", [])
        if not nodes:
            return None
        node = doc["nodes"][nodes[0]]
        prim = doc["meshes"][node["mesh"]]["primitives"][0]
        if prim.get("mode", 4) != 4:
            raise ValueError("not a triangle list")
        att = prim["attributes"]
        pos = self.accessor(att["POSITION"]).astype(np.float64)
        pos = pos * np.asarray(node.get("scale", [1, 1, 1]), np.float64) \
            + np.asarray(node.get("translation", [0, 0, 0]), np.float64)
        return dict(positions=pos,
                    normals=self.accessor(att["NORMAL"]) if "NORMAL" in att else None,
                    colors=self.accessor(att["COLOR_0"]) if "COLOR_0" in att else None,
                    faces=self.accessor(prim["indices"]).reshape(-1, 3))
