"""Marching cubes (csrc/mcubes.hip) and forward_vertices / paint / vertex_points / visualize (csrc/vertices.hip) on
the volumes of tests/surface_cases.py: every one of the 256 corner cases, ties at the level, hits at every border of
the box and in every scan segment, plateaus, zero-length normals, non-finite entries, r = 1 .. 3.

Both files are built with contraction off and claim the op order of the CPU oracle, so everything is held on the
bits (surface_cases.same_bits: NaN for NaN, the same 32 bits elsewhere), not to a tolerance a contracted FMA or a
reordered world_coord would pass.  tests/test_surface_cases_cpu.py shows what the volumes contain and pins the oracle
to the reference's forward_vertices and to float64.  Needs an MI355X."""
import functools

import numpy as np
import pytest

import surface_cases as sc
from monoport_amd import synthetic as syn
from test_box_threshold_cpu import B_MAX, B_MIN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
UNIT = (np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32))
BOXES = {"unit": UNIT, "B": (B_MIN, B_MAX)}
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def depth_case(r, kind):  # shared, never written to
    return sc.depth_case(r, kind)[0]


@functools.lru_cache(maxsize=None)
def named_volume(name):
    if name.startswith("noise"):
        r = int(name[5:])
        return sc.noise_volume(r, sc.NOISE[r])
    if name == "quarters17":
        return sc.quarters_volume(*sc.QUARTERS)
    if name == "nonfinite20":
        return sc.nonfinite_volume(*sc.NONFINITE)
    if name == "blob33":
        return syn.blob_volume(33, 5)
    if name == "sphere65":
        return syn.sphere_volume(65)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------
# marching cubes against oracle.marching_cubes
# ---------------------------------------------------------------------------------------------------------------
def capacities(r):
    return 3 * r ** 3, 5 * (r - 1) ** 3  # every edge crossing, five triangles in every cell


def cut(raw):
    """(verts, faces, counts) of capacity size -> the numpy mesh; the counts must fit the capacity."""
    verts, faces, counts = raw
    nv, nf = counts.cpu().tolist()
    assert nv <= verts.shape[0] and nf <= faces.shape[0], (nv, nf)
    return verts[:nv].cpu().numpy(), faces[:nf].cpu().numpy()


def check_mesh(got, want, what):
    (v, f), (rv, rf) = got, want
    assert v.shape == rv.shape and f.shape == rf.shape, "%s: %s vertices %s faces, expected %s and %s" % (
        what, v.shape, f.shape, rv.shape, rf.shape)
    assert f.dtype == np.int32 and np.array_equal(f, rf), "%s: faces differ" % what
    sc.same_bits(v, rv, what + " vertices")


def test_every_corner_case_as_a_single_cell(ops, oracle):
    """The 256 rows of kMcTriCount / kMcTriEdges one by one: volume c is the one cell of case c."""
    vols = sc.one_cell_volumes()
    max_v, max_f = capacities(2)
    assert ops.MAX_FRAMES == 32
    faces_seen = 0
    for c0 in range(0, 256, ops.MAX_FRAMES):
        raws = ops.marching_cubes_raw_batch([dev(vols[c]) for c in range(c0, c0 + ops.MAX_FRAMES)], 0.5, *UNIT,
                                            max_verts=max_v, max_faces=max_f)
        for k, raw in enumerate(raws):
            case = c0 + k
            want = oracle.marching_cubes(vols[case], 0.5, *UNIT)
            assert raw[2].cpu().tolist() == [len(want[0]), len(want[1])], "case %d: counts" % case
            check_mesh(cut(raw), want, "case %d" % case)
            faces_seen += len(want[1])
    assert faces_seen == 820


@pytest.mark.parametrize("box", ["unit", "B"])
@pytest.mark.parametrize("level", [0.5, 0.3])
@pytest.mark.parametrize("name", ["noise13", "noise17"])
def test_marching_cubes_on_noise(ops, oracle, name, level, box):
    vol = named_volume(name)
    r = vol.shape[0]
    bmin, bmax = BOXES[box]
    max_v, max_f = capacities(r)
    got = cut(ops.marching_cubes_raw(dev(vol), level, bmin, bmax, max_verts=max_v, max_faces=max_f))
    want = oracle.marching_cubes(vol, level, bmin, bmax)
    assert len(want[0]) > 12 * r * r  # more than the default capacity holds
    if level == 0.5:
        assert len(np.unique(sc.corner_cases(vol, level))) == 256
    check_mesh(got, want, "%s level %g box %s" % (name, level, box))


def test_marching_cubes_retry_with_exact_capacities(ops, oracle):
    """recon.marching_cubes on noise13: the default capacity 12 r^2 is too short, the second call gets the counts."""
    from monoport_amd.recon import marching_cubes
    vol = named_volume("noise13")
    want = oracle.marching_cubes(vol, 0.5, B_MIN, B_MAX)
    assert len(want[0]) > 12 * 13 * 13
    v, f = marching_cubes(dev(vol)[None, None], 0.5, B_MIN, B_MAX)
    check_mesh((v.cpu().numpy(), f.cpu().numpy()), want, "noise13 through recon.marching_cubes")


@pytest.mark.parametrize("level", [0.25, 0.5, 0.75])
def test_marching_cubes_ties_at_the_level(ops, oracle, level):
    """Nodes exactly at the level are outside (inside is strictly above it)."""
    vol = named_volume("quarters17")
    assert (vol == np.float32(level)).sum() > 900
    got = cut(ops.marching_cubes_raw(dev(vol), level, B_MIN, B_MAX, max_verts=capacities(17)[0],
                                     max_faces=capacities(17)[1]))
    check_mesh(got, oracle.marching_cubes(vol, level, B_MIN, B_MAX), "quarters17 level %g" % level)


def test_marching_cubes_on_non_finite_values(ops, oracle):
    """NaN and -inf are outside, +inf is inside; an edge that ends in NaN or -inf has a NaN vertex, one that ends in
    +inf has its vertex at the finite end."""
    vol = named_volume("nonfinite20")
    with np.errstate(invalid="ignore", divide="ignore"):
        want = oracle.marching_cubes(vol, 0.5, B_MIN, B_MAX)
    nan_rows = int(np.isnan(want[0]).any(1).sum())
    print("nonfinite20: %d of %d vertices are NaN" % (nan_rows, len(want[0])))
    assert nan_rows >= 200 and not np.isinf(want[0]).any()
    got = cut(ops.marching_cubes_raw(dev(vol), 0.5, B_MIN, B_MAX, max_verts=capacities(20)[0],
                                     max_faces=capacities(20)[1]))
    check_mesh(got, want, "nonfinite20")


def test_marching_cubes_batch_with_trivial_and_gated_frames(ops, oracle):
    vols = [sc.noise_volume(13, 31), np.zeros((13, 13, 13), np.float32), sc.noise_volume(13, 32),
            np.ones((13, 13, 13), np.float32), sc.noise_volume(13, 33)]
    gates = [None, None, torch.zeros(1, dtype=torch.int32, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV),
             torch.full((1,), 7, dtype=torch.int32, device=DEV)]
    max_v, max_f = capacities(13)
    verts = torch.full((5, max_v, 3), SENTINEL, device=DEV)
    faces = torch.full((5, max_f, 3), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((5, 2), -7, dtype=torch.int32, device=DEV)
    raws = ops.marching_cubes_raw_batch([dev(v) for v in vols], 0.5, B_MIN, B_MAX, gates=gates,
                                        out=(verts, faces, counts))
    for k in (1, 2, 3):
        assert raws[k][2].cpu().tolist() == [0, 0], k
    for k in (0, 4):
        check_mesh(cut(raws[k]), oracle.marching_cubes(vols[k], 0.5, B_MIN, B_MAX), "frame %d" % k)
    # nothing of the gated frame was written, and no frame wrote beyond its counts
    for k in range(5):
        nv, nf = counts[k].cpu().tolist()
        assert bool((verts[k, nv:] == SENTINEL).all()) and bool((faces[k, nf:] == -7).all()), k


@pytest.mark.parametrize("name", ["blob33", "sphere65"])
def test_smooth_bodies_on_the_bits(ops, oracle, name):
    """The meshes the other tests hold to 1e-6, held on the bits."""
    from monoport_amd.recon import marching_cubes
    vol = named_volume(name)
    for bmin, bmax in BOXES.values():
        v, f = marching_cubes(dev(vol)[None, None], 0.5, bmin, bmax)
        check_mesh((v.cpu().numpy(), f.cpu().numpy()), oracle.marching_cubes(vol, 0.5, bmin, bmax), name)


# ---------------------------------------------------------------------------------------------------------------
# forward_vertices against oracle.forward_vertices
# ---------------------------------------------------------------------------------------------------------------
def check_rows(raw, want, what):
    """Capacity-sized (X, Y, Z, norm, count) against the oracle's rows; returns the count."""
    x, y, z, n, count = raw
    rx, ry, rz, rn = want
    c = int(count.item())
    assert c == len(rx), "%s: %d rows, expected %d" % (what, c, len(rx))
    assert x.dtype == torch.int64 and y.dtype == torch.int64
    assert np.array_equal(x[:c].cpu().numpy(), rx) and np.array_equal(y[:c].cpu().numpy(), ry), what + ": X, Y"
    sc.same_bits(z[:c].cpu().numpy(), rz, what + " Z")
    sc.same_bits(n[:c].cpu().numpy(), rn, what + " normals")
    return c


def oracle_rows(oracle, vol, direction):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return oracle.forward_vertices(vol, direction)


@pytest.mark.parametrize("direction", sc.DIRECTIONS)
@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("r", [40, 65])
def test_forward_vertices_at_borders_plateaus_and_ties(ops, oracle, r, kind, direction):
    vol = depth_case(r, kind)
    want = oracle_rows(oracle, vol, direction)
    c = check_rows(ops.forward_vertices_raw(dev(vol), direction), want, "depth%d %s %s" % (r, kind, direction))
    assert c > 1000 and (want[0] < 2).sum() >= 50 and (want[1] < 2).sum() >= 50


@pytest.mark.parametrize("direction", ["front", "right"])
@pytest.mark.parametrize("r", [1, 2, 3, 31, 32, 33])
def test_forward_vertices_at_tiny_sizes_and_around_one_segment(ops, oracle, r, direction):
    vol = sc.noise_volume(r, 200 + r)
    if r == 1:
        vol[:] = 0.75  # the single voxel is a hit
    want = oracle_rows(oracle, vol, direction)
    assert len(want[0]) >= 1
    check_rows(ops.forward_vertices_raw(dev(vol), direction), want, "noise%d %s" % (r, direction))


@pytest.mark.parametrize("direction", sc.DIRECTIONS)
def test_forward_vertices_on_non_finite_values(ops, oracle, direction):
    vol = named_volume("nonfinite20")
    want = oracle_rows(oracle, vol, direction)
    assert np.isnan(want[3]).any(1).sum() >= 20 and np.isfinite(want[2]).sum() >= 100
    check_rows(ops.forward_vertices_raw(dev(vol), direction), want, "nonfinite20 " + direction)


def prefilled_forward_vertices(ops, vols, direction):
    """mp_forward_vertices_batch into buffers full of a sentinel (ops.forward_vertices_raw_batch allocates its own)."""
    n, r = len(vols), vols[0].shape[0]
    cap = r * r
    ctx = ops.get_context(vols[0].device)
    x = torch.full((n, cap), -7, dtype=torch.int64, device=DEV)
    y = torch.full((n, cap), -7, dtype=torch.int64, device=DEV)
    z = torch.full((n, cap), SENTINEL, device=DEV)
    nrm = torch.full((n, cap, 3), SENTINEL, device=DEV)
    count = torch.full((n, 1), -7, dtype=torch.int32, device=DEV)
    ctx.check(ctx.lib.mp_forward_vertices_batch(
        ctx.handle, n, ops._ptr_array(vols), r, ops.DIRECTIONS[direction], ops._ptr_array(x), ops._ptr_array(y),
        ops._ptr_array(z), ops._ptr_array(nrm), ops._ptr_array(count), ops._stream(vols[0])),
        "mp_forward_vertices_batch")
    torch.cuda.synchronize()
    return x, y, z, nrm, count


@pytest.mark.parametrize("direction", ["front", "left"])
def test_forward_vertices_batch_frame_by_frame(ops, oracle, direction):
    r = 40
    vols = [depth_case(r, "smooth"), depth_case(r, "binary"), np.zeros((r, r, r), np.float32),
            depth_case(r, "quant"), np.ones((r, r, r), np.float32)]
    raws = ops.forward_vertices_raw_batch([dev(v) for v in vols], direction)
    x, y, z, nrm, count = prefilled_forward_vertices(ops, [dev(v) for v in vols], direction)
    for k, vol in enumerate(vols):
        want = oracle_rows(oracle, vol, direction)
        c = check_rows(raws[k], want, "frame %d %s" % (k, direction))
        assert c == check_rows((x[k], y[k], z[k], nrm[k], count[k]), want, "prefilled frame %d %s" % (k, direction))
        # rows beyond the count stay untouched
        assert bool((x[k, c:] == -7).all()) and bool((y[k, c:] == -7).all())
        assert bool((z[k, c:] == SENTINEL).all()) and bool((nrm[k, c:] == SENTINEL).all())
    assert int(count[2].item()) == 0 and int(count[4].item()) == r * r
    assert bool(torch.isnan(z[4]).all())  # every column hits at z' = 0: 0/0


# ---------------------------------------------------------------------------------------------------------------
# what consumes those rows: paint, vertex_points, visualize
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,direction", [("smooth", "front"), ("binary", "back"), ("quant", "left")])
def test_paint_of_edge_rows(ops, oracle, kind, direction):
    r = 40
    vol = depth_case(r, kind)
    rx, ry, rz, rn = oracle_rows(oracle, vol, direction)
    x, y, z, n, count = ops.forward_vertices_raw(dev(vol), direction)
    img = ops.paint(x, y, n, 0, count, r, 0.5, 0.5, 0.0, 1.0).cpu().numpy()
    want = oracle.colorization(rx, ry, rz, r, norm=rn)
    sc.same_bits(img, want, "paint %s %s" % (kind, direction))
    painted = np.zeros((r, r), bool)
    painted[rx, ry] = True
    assert (~painted).sum() >= 20 and (img[~painted] == 1.0).all()
    if kind == "binary":
        assert np.isnan(img).all(2).sum() >= 100  # zero-length normals give NaN pixels
        assert np.array_equal(np.isnan(img[rx, ry]), np.isnan(rn))


@pytest.mark.parametrize("direction", ["front", "back"])
def test_vertex_points_of_edge_rows(ops, oracle, direction):
    """NaN exactly where Z is NaN (0 * NaN in the rows of the other axes too), ops.orthogonal's bits elsewhere."""
    from monoport_amd.recon import color_matrix
    r = 40
    vol = depth_case(r, "smooth")
    x, y, z, _, count = ops.forward_vertices_raw(dev(vol), direction)
    c = int(count.item())
    m = color_matrix(B_MIN, B_MAX, r)
    pts = ops.vertex_points(x, y, z, count, r, m)[:, :c]
    verts = torch.stack([x[:c].float(), y[:c].float(), float(r) - z[:c]])
    orth = ops.orthogonal(verts[None].contiguous(), dev(m)[None])[0]
    p, zz = pts.cpu().numpy(), z[:c].cpu().numpy()
    assert 50 <= np.isnan(zz).sum() <= c - 100
    assert np.array_equal(np.isnan(p), np.broadcast_to(np.isnan(zz), (3, c)))
    sc.same_bits(p, orth.cpu().numpy(), "vertex_points " + direction)
    ok = ~np.isnan(zz)
    for k, col in enumerate((x[:c].cpu().numpy(), y[:c].cpu().numpy(), np.float32(r) - zz)):
        own = ((m[k, k] * col.astype(np.float32)).astype(np.float32) + m[k, 3]).astype(np.float32)
        assert np.array_equal(p[k][ok], own[ok]), k


@pytest.mark.parametrize("size", [64, 37])
def test_visulization_of_a_canvas_with_nan_pixels(ops, size):
    """RTL/main.py:252-281 restated with stock tensor ops on the CPU, at an integer-free scale (40 -> 37) too; a NaN
    pixel is not white, so it counts as foreground."""
    import torch.nn.functional as F
    from monoport_amd.recon import visulization
    r = 40
    x, y, z, n, count = ops.forward_vertices_raw(dev(depth_case(r, "binary")), "back")
    canvas = ops.paint(x, y, n, 0, count, r, 0.5, 0.5, 0.0, 1.0)
    t = canvas.cpu()
    assert int(torch.isnan(t).all(2).sum()) >= 100 and int((t == 1).all(2).sum()) >= 20
    ref = torch.rot90(t * 255.0, 1, [0, 1]).permute(2, 0, 1).unsqueeze(0)
    ref = F.interpolate(ref, size=(size, size))[0].numpy().transpose(1, 2, 0)
    bg = (ref == 255).all(2)
    out, tex, mask = visulization(canvas, None, render_size=size)
    assert tex is None and out.shape == (size, size, 3)
    assert np.array_equal(out, ref, equal_nan=True)
    assert np.isnan(ref).any() and bg.any()
    assert np.array_equal(mask, ~bg.reshape(size, size, 1))
    assert mask[np.isnan(ref).all(2)].all()
