"""Per-vertex mesh normals (mesh_util.compute_normal, numpy path) against the reference's compute_normal, and
the OBJ-with-normals writer against the reference's reader -- both through tests/golden/mesh_normals.npz
(tools/gen_golden_mesh.py), so neither a GPU nor the reference is needed."""
import os

import numpy as np
import pytest
import torch

from monoport_amd import mesh_util
from monoport_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_normals.npz")
CASES = [("blob33", 32), ("blob33", 64), ("sphere65", 32), ("soup", 32), ("soup", 64)]


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def mesh_of(golden, name):
    if name == "soup":
        v, f, _ = syn.normals_soup_mesh()
        return v, f
    return golden[name + "_verts"], golden[name + "_faces"]


def accumulate_model(v, f):
    """The accumulate definition restated: every (face, corner) adds the face's unit normal, unbuffered and in
    ascending order (np.add.at), f32 / f64 adds starting from +0; then normalize_v3."""
    def normalize_v3(a):
        lens = np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2 + a[:, 2] ** 2)
        lens[lens < a.dtype.type(1e-8)] = a.dtype.type(1e-8)
        return a / lens[:, None]
    t = v[f]
    n = normalize_v3(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]))
    out = np.zeros_like(v)
    np.add.at(out, f.reshape(-1), np.repeat(n, 3, axis=0))
    return normalize_v3(out)


def angle_deg(a, b):
    return np.degrees(np.arccos(np.clip((a.astype(np.float64) * b.astype(np.float64)).sum(1), -1.0, 1.0)))


def test_fixture_meshes_regenerate_from_seeds(golden):
    from oracle import pifu_oracle as orc
    for name, vol in (("blob33", syn.blob_volume(33, 5)), ("sphere65", syn.sphere_volume(65))):
        v, f = orc.marching_cubes(vol)
        assert np.array_equal(v, golden[name + "_verts"]) and np.array_equal(f, golden[name + "_faces"]), name
    v, f, centre = syn.normals_soup_mesh()
    assert golden["soup_ref32"].shape == v.shape and np.bincount(f.reshape(-1))[centre] >= 200


@pytest.mark.parametrize("name,bits", CASES)
def test_reference_mode_equals_the_reference_bit_for_bit(golden, name, bits):
    v, f = mesh_of(golden, name)
    v = v.astype(np.float32 if bits == 32 else np.float64)
    keep_v, keep_f = v.copy(), f.copy()
    out = mesh_util.compute_normal(v, f)  # the drop-in's default is the reference's behaviour
    assert isinstance(out, np.ndarray) and out.dtype == v.dtype
    assert np.array_equal(out, golden["%s_ref%d" % (name, bits)])
    assert not np.isnan(out).any()
    assert np.array_equal(v, keep_v) and np.array_equal(f, keep_f)


@pytest.mark.parametrize("name,bits", CASES)
def test_accumulate_mode_equals_add_at_bit_for_bit(golden, name, bits):
    v, f = mesh_of(golden, name)
    v = v.astype(np.float32 if bits == 32 else np.float64)
    keep_v, keep_f = v.copy(), f.copy()
    out = mesh_util.compute_normal(v, f, mode="accumulate")
    assert out.dtype == v.dtype and np.array_equal(out, accumulate_model(v, f.astype(np.int64)))
    assert not np.isnan(out).any()
    assert np.array_equal(v, keep_v) and np.array_equal(f, keep_f)


@pytest.mark.parametrize("mode", ["reference", "accumulate"])
def test_degenerate_faces_and_unreferenced_vertices_give_exact_zeros(mode):
    v, f, centre = syn.normals_soup_mesh()
    out = mesh_util.compute_normal(v, f, mode)
    valence = np.bincount(f.reshape(-1), minlength=len(v))
    assert (valence == 0).sum() >= 4
    assert (out[valence == 0] == 0).all() and not np.isnan(out).any()
    # vertices 500..502 are exactly collinear and sit in zero-area faces only
    assert (out[500:503] == 0).all()
    # a mesh of degenerate faces alone: every normal is 0 / 1e-8 = 0
    deg = np.array([[0, 0, 1], [2, 2, 2], [500, 501, 502]], np.int32)
    assert (mesh_util.compute_normal(v, deg, mode) == 0).all()
    # the fan's centre has a proper unit normal
    assert abs(np.linalg.norm(out[centre].astype(np.float64)) - 1) < 1e-6


def test_accumulate_is_closer_to_the_radial_direction_on_the_sphere(golden):
    """The two modes are different functions and cannot be swapped silently: a comparison of two measured
    medians, no threshold."""
    v, f = mesh_of(golden, "sphere65")
    rad = v.astype(np.float64)
    rad /= np.linalg.norm(rad, axis=1)[:, None]
    ref = np.median(angle_deg(mesh_util.compute_normal(v, f, "reference"), rad))
    acc = np.median(angle_deg(mesh_util.compute_normal(v, f, "accumulate"), rad))
    print("median angle to the radial direction: reference %.3f deg, accumulate %.3f deg" % (ref, acc))
    assert acc < ref


def test_tensor_in_tensor_out_and_bad_arguments(golden):
    v, f = mesh_of(golden, "blob33")
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    out = mesh_util.compute_normal(tv, tf)
    assert torch.is_tensor(out) and out.dtype == torch.float32 and out.device == tv.device
    assert np.array_equal(out.numpy(), golden["blob33_ref32"])
    out64 = mesh_util.compute_normal(tv.double(), tf, "reference")
    assert out64.dtype == torch.float64 and np.array_equal(out64.numpy(), golden["blob33_ref64"])
    assert np.array_equal(tv.numpy(), v) and np.array_equal(tf.numpy(), f)
    assert mesh_util.compute_normal(v, np.zeros((0, 3), np.int32), "accumulate").tolist() == np.zeros_like(v).tolist()
    with pytest.raises(ValueError):
        mesh_util.compute_normal(v, f, mode="area")
    with pytest.raises(ValueError):
        mesh_util.compute_normal(v[:, :2], f)


def parse_obj(path):
    """A short OBJ reader: v / vn rows and the two index columns of ``f a//b`` corners, zero-based."""
    vs, cs, ns, fv, fn = [], [], [], [], []
    for line in open(path):
        t = line.split()
        if t[0] == "v":
            vs.append([float(x) for x in t[1:4]])
            cs.append([float(x) for x in t[4:7]])
        elif t[0] == "vn":
            ns.append([float(x) for x in t[1:4]])
        elif t[0] == "f":
            parts = [c.split("/") for c in t[1:4]]
            assert all(len(p) == 3 and p[1] == "" for p in parts), line
            fv.append([int(p[0]) - 1 for p in parts])
            fn.append([int(p[2]) - 1 for p in parts])
    return np.array(vs), np.array(cs), np.array(ns), np.array(fv), np.array(fn)


def test_obj_with_normals_loads_as_the_reference_reader_loads_it(golden, tmp_path):
    v, f = mesh_of(golden, "blob33")
    normals = mesh_util.compute_normal(v, f, "accumulate")
    path = tmp_path / "n.obj"
    mesh_util.save_obj_mesh_with_normals(str(path), v, f, normals)
    lines = open(path).read().splitlines()
    assert len(lines) == 2 * len(v) + len(f)
    assert [l.split()[0] for l in lines] == ["v"] * len(v) + ["vn"] * len(v) + ["f"] * len(f)
    vs, _, ns, fv, fn = parse_obj(path)
    assert np.array_equal(vs, golden["obj_verts"])
    assert np.array_equal(fv, golden["obj_faces"]) and np.array_equal(fn, golden["obj_face_normals"])
    assert np.array_equal(fv, f) and np.array_equal(fn, f)
    # the reference's reader renormalises the vn rows (normalize_v3 in float64)
    lens = np.sqrt(ns[:, 0] ** 2 + ns[:, 1] ** 2 + ns[:, 2] ** 2)
    lens[lens < 1e-8] = 1e-8
    assert np.array_equal(ns / lens[:, None], golden["obj_norms"])
    # and what was written is the normals to the 4 decimals of the format
    assert np.abs(ns - normals).max() <= 0.5e-4 + 1e-7


def test_obj_with_normals_and_colours_keeps_the_colour_writer_v_lines(tmp_path):
    v, f, c = syn.obj_mesh_inputs()
    normals = mesh_util.compute_normal(v, f, "accumulate")
    p1, p2 = tmp_path / "c.obj", tmp_path / "cn.obj"
    mesh_util.save_obj_mesh_with_color(str(p1), v, f, c)
    mesh_util.save_obj_mesh_with_normals(str(p2), torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(normals),
                                         colors=c)
    l1, l2 = open(p1).read().splitlines(), open(p2).read().splitlines()
    assert l2[:len(v)] == l1[:len(v)]
    assert l2[len(v)] == "vn %.4f %.4f %.4f" % tuple(normals[0])
    i, j, k = (int(a) + 1 for a in f[0])
    assert l2[2 * len(v)] == "f %d//%d %d//%d %d//%d" % (i, i, j, j, k, k)
    assert len(l2) == 2 * len(v) + len(f)
