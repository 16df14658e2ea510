"""The textured binary glTF file of mp_mesh_glb_textured (include/monoport_hip.h) restated in numpy, byte for byte, on top
of tests/glb_ref.py (container, quantisation), tests/atlas_ref.py (the UVs) and tests/png_ref.py (the image); and the
reading side by the glTF 2.0 specification alone: ``read`` follows material -> texture -> image -> buffer view, and
``viewer_colours`` does what a viewer does with TEXCOORD_0 and the decoded image."""
import io
import struct

import numpy as np

import atlas_ref
import glb_ref as ref
import png_ref

F = np.float32
PNG_MIN_BYTES = png_ref.MIN_BYTES


def _number(v, width):
    return ("%d" % v).rjust(width)


def bin_layout(nf, normals, png_bytes):
    off_n = 24 * nf
    off_t = off_n + (12 * nf if normals else 0)
    off_img = off_t + 24 * nf
    return dict(off_n=off_n, off_t=off_t, off_img=off_img, img=png_bytes, bin=(off_img + png_bytes + 3) // 4 * 4)


def json_text(normals, b_min, b_max, nf, qmin, qmax, layout):
    """The JSON chunk's text (padded) of a non-empty textured mesh."""
    nrm = bool(normals)
    c = 1 + nrm
    k = c + 1
    b_min, b_max = np.asarray(b_min, F).astype(np.float64), np.asarray(b_max, F).astype(np.float64)
    real = lambda x: "%24.17g" % x  # noqa: E731
    t = ref.ASSET + ',"extensionsUsed":["KHR_mesh_quantization"],"extensionsRequired":["KHR_mesh_quantization"]'
    t += ',"scene":0,"scenes":[{"nodes":[0]}],"nodes":[{"mesh":0,"translation":['
    t += ",".join(real(b_min[a]) for a in range(3)) + '],"scale":['
    t += ",".join(real((b_max[a] - b_min[a]) / 65535.0) for a in range(3))
    t += ']}],"materials":[{"doubleSided":true,"pbrMetallicRoughness":{"baseColorTexture":{"index":0},'
    t += '"metallicFactor":0,"roughnessFactor":1}}],"textures":[{"sampler":0,"source":0}],'
    t += '"samplers":[{"magFilter":9729,"minFilter":9729,"wrapS":33071,"wrapT":33071}],'
    t += '"images":[{"bufferView":%d,"mimeType":"image/png"}],' % k
    t += '"meshes":[{"primitives":[{"attributes":{"POSITION":0'
    if nrm:
        t += ',"NORMAL":1'
    t += ',"TEXCOORD_0":%d},"material":0,"mode":4}]}],"accessors":[' % c
    nc = _number(3 * nf, 10)
    t += '{"bufferView":0,"componentType":5123,"count":%s,"type":"VEC3","min":[%s],"max":[%s]}' % (
        nc, ",".join(_number(v, 5) for v in qmin), ",".join(_number(v, 5) for v in qmax))
    if nrm:
        t += ',{"bufferView":1,"componentType":5120,"normalized":true,"count":%s,"type":"VEC3"}' % nc
    t += ',{"bufferView":%d,"componentType":5126,"count":%s,"type":"VEC2"}],"bufferViews":[' % (c, nc)
    view = '{"buffer":0,"byteOffset":%s,"byteLength":%s'
    t += view % (_number(0, 10), _number(24 * nf, 10)) + ',"byteStride":8,"target":34962}'
    if nrm:
        t += "," + view % (_number(layout["off_n"], 10), _number(12 * nf, 10)) + ',"byteStride":4,"target":34962}'
    t += "," + view % (_number(layout["off_t"], 10), _number(24 * nf, 10)) + ',"byteStride":8,"target":34962}'
    t += "," + view % (_number(layout["off_img"], 10), _number(layout["img"], 10)) + "}"
    t += '],"buffers":[{"byteLength":%s}]}' % _number(layout["bin"], 10)
    return t + " " * ((12 - len(t) % 8) % 8)


def json_len(normals):
    z = (0, 0, 0)
    return len(json_text(normals, z, (1, 1, 1), 1, z, z, bin_layout(1, normals, 57)))


def file_bytes(nf, png_bytes, normals=True):
    """mp_glb_textured_bytes."""
    if nf == 0:
        return ref.MIN_BYTES
    return 12 + 8 + json_len(normals) + 8 + bin_layout(nf, normals, png_bytes)["bin"]


def max_bytes(max_faces, size, normals=True):
    """mp_glb_textured_max_bytes."""
    return file_bytes(max_faces, png_ref.max_bytes(size, size, "rgb8"), normals)


def encode(verts, faces, size, cell, png, counts=None, normals=None, b_min=(-1, -1, -1), b_max=(1, 1, 1),
           png_overflowed=False, capacity=None):
    """-> (file bytes or None where nothing is written, info (bytes, code)).  ``png``: the bytes of the atlas's PNG."""
    verts, faces = np.asarray(verts, F).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    counts = (len(verts), len(faces)) if counts is None else counts
    nv = min(max(int(counts[0]), 0), len(verts))
    nf = min(max(int(counts[1]), 0), len(faces))
    if nv == 0 or nf == 0:
        data = ref.encode(verts, faces, (0, 0))
    elif nf > atlas_ref.capacity(size, cell) or png_overflowed or len(png) < PNG_MIN_BYTES:
        return None, (0, 2)
    else:
        layout = bin_layout(nf, normals is not None, len(png))
        corner = np.clip(faces[:nf].astype(np.int64), 0, nv - 1).reshape(-1)
        q = ref.quantise_positions(verts[corner], b_min, b_max)
        pos = np.zeros((3 * nf, 4), "<u2")
        pos[:, :3] = q
        data = pos.tobytes()
        if normals is not None:
            rows = np.zeros((3 * nf, 4), np.uint8)
            rows[:, :3] = ref.quantise_normals(np.asarray(normals, F).reshape(-1, 3)[corner]) & 0xFF
            data += rows.tobytes()
        data += atlas_ref.corner_uvs(nf, size, cell).astype("<f4").tobytes()
        data += bytes(png)
        data += b"\0" * (-len(data) % 4)
        assert len(data) == layout["bin"]
        text = json_text(normals is not None, b_min, b_max, nf, q.min(axis=0), q.max(axis=0), layout).encode("ascii")
        body = ref._chunk(b"JSON", text) + ref._chunk(b"BIN\0", data)
        data = struct.pack("<4sII", b"glTF", 2, 12 + len(body)) + body
    if capacity is not None and len(data) > capacity:
        return None, (len(data), 1)
    return data, (len(data), 0)


# ---- the reader: the glTF 2.0 specification, nothing of the above -----------------------------------------------------
def read(data):
    """A textured file by the specification: dict with ``positions`` [n,3] float64 in world coordinates, ``normals`` or
    None, ``uv`` [n,2], ``faces`` [n/3,3] (an unindexed triangle list: consecutive vertices), ``png`` (the image's
    bytes), ``sampler`` (its dict), ``doc`` (the JSON); None for a file without nodes."""
    g = ref.Glb(data)
    doc = g.json
    nodes = doc["scenes"][doc.get("scene", 0)].get("nodes", [])
    if not nodes:
        return None
    node = doc["nodes"][nodes[0]]
    prim = doc["meshes"][node["mesh"]]["primitives"][0]
    if prim.get("mode", 4) != 4:
        raise ValueError("not a triangle list")
    att = prim["attributes"]
    pos = g.accessor(att["POSITION"]).astype(np.float64)
    n = len(pos)
    if "indices" in prim:
        faces = g.accessor(prim["indices"]).reshape(-1, 3)
    else:
        if n % 3:
            raise ValueError("an unindexed triangle list of %d vertices" % n)
        faces = np.arange(n, dtype=np.int64).reshape(-1, 3)
    acc = doc["accessors"][att["POSITION"]]
    raw = g.accessor(att["POSITION"], raw=True)
    if list(raw.min(axis=0)) != acc["min"] or list(raw.max(axis=0)) != acc["max"]:
        raise ValueError("POSITION's min / max are not its extremes")
    pos = pos * np.asarray(node.get("scale", [1, 1, 1]), np.float64) \
        + np.asarray(node.get("translation", [0, 0, 0]), np.float64)
    material = doc["materials"][prim["material"]]
    info = material["pbrMetallicRoughness"]["baseColorTexture"]
    if info.get("texCoord", 0) != 0 or "COLOR_0" in att:
        raise ValueError("the texture is expected on TEXCOORD_0, without vertex colours")
    texture = doc["textures"][info["index"]]
    image = doc["images"][texture["source"]]
    if image["mimeType"] != "image/png" or "uri" in image:
        raise ValueError("the image is expected as a PNG in a buffer view")
    view = doc["bufferViews"][image["bufferView"]]
    if "byteStride" in view or "target" in view:
        raise ValueError("an image's buffer view has neither a stride nor a target")
    start = view.get("byteOffset", 0)
    if view["buffer"] != 0 or start + view["byteLength"] > doc["buffers"][0]["byteLength"]:
        raise ValueError("the image leaves the buffer")
    uv = g.accessor(att["TEXCOORD_0"])
    for name in ("NORMAL", "TEXCOORD_0"):
        if name in att and doc["accessors"][att[name]]["count"] != n:
            raise ValueError("%s has another count than POSITION" % name)
    return dict(positions=pos, normals=g.accessor(att["NORMAL"]) if "NORMAL" in att else None,
                uv=uv.astype(np.float64), faces=faces, png=bytes(g.bin[start:start + view["byteLength"]]),
                sampler=doc["samplers"][texture["sampler"]], doc=doc)


def decode_png(data):
    """The image of a PNG file by Pillow: uint8 [H,W,3]."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    if im.mode != "RGB":
        raise ValueError("an RGB image is expected, got mode %s" % im.mode)
    return np.asarray(im)


def viewer_colours(parsed, face, bary):
    """What a viewer shows at the surface points (face [n], barycentric weights [n,3]) of a ``read`` file: the UVs of
    the face's three vertices interpolated, the decoded image looked up under the file's sampler (LINEAR, clamped),
    base colour factor 1: float64 [n,3] in 0..1; and the points' positions [n,3] from the file."""
    s = parsed["sampler"]
    if (s.get("magFilter"), s.get("minFilter"), s.get("wrapS"), s.get("wrapT")) != (9729, 9729, 33071, 33071):
        raise ValueError("a LINEAR sampler without mips, clamped, is expected: %r" % s)
    image = decode_png(parsed["png"]).astype(np.float64) / 255.0
    if image.shape[0] != image.shape[1]:
        raise ValueError("a square atlas is expected")
    idx = parsed["faces"][face]  # [n,3]
    uv = (parsed["uv"][idx] * bary[:, :, None]).sum(axis=1)
    pos = (parsed["positions"][idx] * bary[:, :, None]).sum(axis=1)
    return atlas_ref.sample_bilinear(image, uv), pos
