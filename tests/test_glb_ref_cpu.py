"""The numpy restatement of the binary glTF definition (tests/glb_ref.py), read back by the independent reader of the
same module, which follows the glTF 2.0 specification alone: container, JSON, alignment, sizes, faces, and the
quantisation bounds of every attribute.  No GPU."""
import json
import struct

import numpy as np
import pytest

import glb_cases as cases
import glb_ref as ref

F = np.float32
ALL = cases.small_cases()
MESHES = [c for c in ALL if min(c.counts) > 0]
EMPTY = [c for c in ALL if min(c.counts) <= 0]


def clamped_counts(c):
    return min(max(c.counts[0], 0), len(c.verts)), min(max(c.counts[1], 0), len(c.faces))


@pytest.mark.parametrize("flags", cases.ATTRIBUTE_SETS, ids=str)
@pytest.mark.parametrize("case", MESHES, ids=lambda c: c.name)
def test_container_and_layout(case, flags):
    data = cases.restated(case, *flags)
    nv, nf = clamped_counts(case)
    g = ref.Glb(data)  # the header's length is the file's, the chunks fill it, json.loads accepts the text
    assert len(data) == ref.file_bytes(nv, nf, *flags) and len(data) % 4 == 0
    assert [k for k, _, _ in g.chunks] == [b"JSON", b"BIN\0"]
    (_, at, text), (_, bin_at, blob) = g.chunks
    assert at == 20 and len(text) == ref.json_len(flags) and len(text) % 4 == 0 and bin_at % 8 == 0
    stripped = text.rstrip(b" ")
    assert stripped.endswith(b"}") and len(text) - len(stripped) < 8
    doc = g.json
    assert doc["asset"]["version"] == "2.0"
    assert doc["extensionsUsed"] == doc["extensionsRequired"] == ["KHR_mesh_quantization"]
    assert doc["scene"] == 0 and doc["scenes"] == [{"nodes": [0]}] and len(doc["nodes"]) == 1
    assert doc["materials"] == [{"doubleSided": True}]
    (prim,) = doc["meshes"][0]["primitives"]
    assert prim["mode"] == 4 and prim["material"] == 0
    assert sorted(prim["attributes"]) == sorted(["POSITION"] + ["NORMAL"] * flags[0] + ["COLOR_0"] * flags[1])
    views = doc["bufferViews"]
    assert len(views) == len(doc["accessors"]) == 2 + flags[0] + flags[1]
    end = 0
    for v in views:  # in order, back to back, each at a multiple of 4
        assert v["byteOffset"] == end and v["byteOffset"] % 4 == 0
        end = v["byteOffset"] + v["byteLength"]
    assert doc["buffers"] == [{"byteLength": len(blob)}] and 0 <= len(blob) - end < 4
    assert blob[end:] == b"\0" * (len(blob) - end)
    assert [v.get("byteStride") for v in views] == [8] + [4] * (flags[0] + flags[1]) + [None]
    # a translation and a scale that take the integers back into the box, in double from the f32 box
    lo, hi = np.asarray(case.b_min, F).astype(np.float64), np.asarray(case.b_max, F).astype(np.float64)
    node = doc["nodes"][0]
    assert node["translation"] == list(lo) and node["scale"] == list((hi - lo) / 65535.0)
    # the padding bytes of the attributes are zero
    pos = np.frombuffer(blob, "<u2", 4 * nv).reshape(nv, 4)
    assert (pos[:, 3] == 0).all()
    for k in range(1, 1 + flags[0] + flags[1]):
        rows = np.frombuffer(blob, np.uint8, 4 * nv, views[k]["byteOffset"]).reshape(nv, 4)
        assert (rows[:, 3] == 0).all()


@pytest.mark.parametrize("case", MESHES, ids=lambda c: c.name)
def test_reader_gives_the_mesh_back(case):
    data = cases.restated(case)
    nv, nf = clamped_counts(case)
    g = ref.Glb(data)
    m = g.mesh()
    assert m["faces"].shape == (nf, 3) and m["positions"].shape == (nv, 3)
    assert np.array_equal(m["faces"], np.clip(case.faces[:nf].astype(np.int64), 0, nv - 1))
    # positions: within 0.52 step per axis of the vertex clamped onto the box (0.5 from the rounding; the two f32
    # operations add at most 65535 * 2^-22 = 0.016 step)
    lo, hi = np.asarray(case.b_min, F).astype(np.float64), np.asarray(case.b_max, F).astype(np.float64)
    step = (hi - lo) / 65535.0
    v = case.verts[:nv].astype(np.float64)
    want = np.clip(np.where(np.isnan(v), lo, v), lo, hi)  # a NaN gives 0: the box's lower bound
    err = np.abs(m["positions"] - want) / step
    print("%s: positions within %.4f step" % (case.name, err.max()))
    assert err.max() <= 0.52
    # POSITION min / max are the extremes of the stored integers
    acc = g.json["accessors"][0]
    q = g.accessor(0, raw=True)
    assert acc["min"] == list(q.min(axis=0)) and acc["max"] == list(q.max(axis=0))
    assert acc["componentType"] == 5123 and "normalized" not in acc and acc["count"] == nv
    # normals: within 0.5 / 127 + 1e-6 of the clamped components
    n = case.normals[:nv].astype(np.float64)
    want = np.clip(np.where(np.isnan(n), 0.0, n), -1.0, 1.0)
    err = np.abs(m["normals"] - want).max()
    print("%s: normals within %.6f" % (case.name, err))
    assert err <= 0.5 / 127 + 1e-6
    # colours: exactly the 8-bit rule of picture_u8
    assert np.array_equal(g.accessor(g.json["meshes"][0]["primitives"][0]["attributes"]["COLOR_0"], raw=True),
                          ref.to_u8(case.colors[:nv]))
    assert g.json["accessors"][2]["normalized"] is True and g.json["accessors"][1]["componentType"] == 5120


def test_the_8_bit_rule():
    x = np.array([-1, -0.0, 0, 0.4999 / 255, 0.5 / 255, 0.50001 / 255, 1 / 255, 127.5 / 255, 254.49 / 255, 254.51 / 255, 1,
                  2, np.inf, -np.inf, np.nan], F)
    with np.errstate(invalid="ignore"):
        want = [int(np.float32(np.float32(min(max(v, 0), 1)) * F(255)) + F(0.5)) if v == v else 0 for v in x]
    assert list(ref.to_u8(x)) == want
    assert list(ref.quantise_colours(np.array([-1, 0, 1, np.nan], F), 0.5, 0.5)) == [0, 128, 255, 0]


def test_colour_layouts_and_the_chain_s_raw_predictions():
    """Planes give the bytes of rows, and the raw predictions with (0.5, 0.5) the bytes of the finished colours."""
    c = cases.small_cases()[3]
    assert cases.restated(c, True, True, "planes") == cases.restated(c)
    raw = ((c.colors - F(0.5)) * F(2)).astype(F)
    finished = (raw * F(0.5) + F(0.5)).astype(F)
    a = ref.encode(c.verts, c.faces, c.counts, c.normals, raw.T.copy(), "planes", 0.5, 0.5, c.b_min, c.b_max)
    b = ref.encode(c.verts, c.faces, c.counts, c.normals, finished, "rows", 1.0, 0.0, c.b_min, c.b_max)
    assert a == b


def test_index_width_switches_between_65535_and_65536():
    narrow, wide = cases.index_width_cases()
    for c, ctype, dtype in ((narrow, 5123, "<u2"), (wide, 5125, "<u4")):
        data = cases.restated(c)
        g = ref.Glb(data)
        nv = len(c.verts)
        acc = g.json["accessors"][-1]
        assert acc["componentType"] == ctype and acc["count"] == 15 and len(data) == ref.file_bytes(nv, 5)
        view = g.json["bufferViews"][-1]
        assert view["byteLength"] == 15 * np.dtype(dtype).itemsize
        faces = g.mesh()["faces"]
        assert np.array_equal(faces, c.faces) and faces.max() == nv - 1
    assert ref.Glb(cases.restated(narrow)).mesh()["faces"].max() == 65534  # 65535 never occurs in a 16-bit file


@pytest.mark.parametrize("case", EMPTY, ids=lambda c: c.name)
def test_the_empty_file(case):
    """nv == 0, nf == 0 and {0, 0} give the one fixed file, whatever the attribute set."""
    files = {cases.restated(case, *flags) for flags in cases.ATTRIBUTE_SETS}
    assert len(files) == 1
    (data,) = files
    assert len(data) == ref.MIN_BYTES == ref.file_bytes(0, 7) == ref.file_bytes(7, 0) == ref.file_bytes(0, 0)
    g = ref.Glb(data)
    assert len(g.chunks) == 1 and g.bin is None and g.mesh() is None
    assert g.json == {"asset": {"version": "2.0", "generator": "monoport_amd"}, "scene": 0, "scenes": [{}]}
    assert data == cases.restated(EMPTY[0])
    assert struct.unpack_from("<I", data, 8)[0] == len(data) and data[20:].rstrip(b" ") == ref.EMPTY_JSON.encode()


def test_the_text_has_one_length_per_attribute_set():
    """Counts of one digit and of ten give texts of one length, and json.loads reads the padded numbers."""
    z = (0, 0, 0)
    for flags in cases.ATTRIBUTE_SETS:
        big = ref.json_text(flags, (-1e-30, -3.0000002, 1e30), (1e-30, 3.0000002, 3e38), 2 ** 28 - 1, 2 ** 28, z,
                            (65535,) * 3, ref.bin_layout(2 ** 28 - 1, 2 ** 28, flags))
        assert len(big) == ref.json_len(flags) and len(big) % 8 == 4
        doc = json.loads(big)
        assert doc["accessors"][0]["count"] == 2 ** 28 - 1 and doc["accessors"][-1]["count"] == 3 * 2 ** 28
    assert ref.json_len((True, True)) > ref.json_len((True, False)) == ref.json_len((False, True)) > ref.json_len(
        (False, False))


def test_the_library_s_closed_form_and_the_glb_options():
    """mp_glb_bytes / mp_glb_max_bytes (host functions of the library) against the restatement, and recon.Glb."""
    from monoport_amd import _lib, ops, recon
    for nv, nf in ((0, 0), (0, 9), (9, 0), (1, 1), (3, 1), (50, 7), (50, 8), (65535, 5), (65536, 5), (86040, 172076)):
        for flags in cases.ATTRIBUTE_SETS:
            assert ops.glb_bytes(nv, nf, *flags) == ref.file_bytes(nv, nf, *flags), (nv, nf, flags)
            assert ops.glb_max_bytes(nv, nf, *flags) == ref.file_bytes(nv, nf, *flags)
    lib = _lib.load()
    assert lib.mp_glb_bytes(-1, 4, 3) == 0 and lib.mp_glb_bytes(4, -1, 3) == 0 and lib.mp_glb_bytes(4, 4, 4) == 0
    assert lib.mp_glb_max_bytes(4, 4, -1) == 0 and ops.GLB_MIN_BYTES == ref.MIN_BYTES
    with pytest.raises(ValueError, match="glb_bytes"):
        ops.glb_bytes(-1, 3)
    g = recon.Glb()
    assert g.normals and g.colors and g.capacity is None
    r = 257
    cap = g.capacity_for(12 * r * r, 24 * r * r)
    assert cap == ref.file_bytes(3 * r * r, 6 * r * r) and cap <= ops.glb_max_bytes(12 * r * r, 24 * r * r)
    assert cap > 2 * ref.file_bytes(86040, 172076)  # the 257^3 body with room to spare
    assert g.capacity_for(3, 3) == ref.MIN_BYTES and recon.Glb(capacity=4096).capacity_for(10 ** 6, 10 ** 6) == 4096
    assert recon.Glb(False, False).capacity_for(400, 800) == ref.file_bytes(100, 200, False, False)
    for bad in (dict(normals=1), dict(colors=None), dict(capacity=99), dict(capacity=2 ** 31 + 1), dict(capacity=4096.0),
                dict(capacity=True)):
        with pytest.raises(ValueError, match="Glb"):
            recon.Glb(**bad)
    with pytest.raises(ValueError, match="recon.Glb"):
        recon.encode_glb([], glb="glb")
    with pytest.raises(ValueError, match="mesh 0 has no colors"):
        recon.encode_glb(recon.Mesh(None, None, 1, None))
    with pytest.raises(ValueError, match="mesh 1 has no normals"):
        recon.encode_glb([recon.Mesh(None, None, 1, None), recon.Mesh(None, None, None, None)], recon.Glb(colors=False))
    assert recon.encode_glb([]) == []


def test_the_reader_refuses_a_damaged_file():
    data = cases.restated(cases.small_cases()[0])
    for bad in (data[:-4], b"glTX" + data[4:], data[:8] + struct.pack("<I", len(data) + 4) + data[12:]):
        with pytest.raises(ValueError):
            ref.Glb(bad)
