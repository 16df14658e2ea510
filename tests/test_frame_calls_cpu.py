"""The per-frame mesh and render wrappers without a GPU: each is its ``_batch`` twin on one-element lists, so it refuses
what the twin refuses before any device call, and the helper that cuts a list of frames into calls of at most
MAX_FRAMES."""
import pytest

torch = pytest.importorskip("torch")


def test_frame_wrappers_check_their_arguments_on_the_host():
    """CPU tensors and no context: a call that reached the library would raise MonoportError (no CPU path), not
    ValueError."""
    from monoport_amd import ops
    v, f = torch.zeros(6, 3), torch.zeros(4, 3, dtype=torch.int32)
    c = torch.zeros(2, dtype=torch.int32)
    slab = torch.zeros(3, 4, 5)
    for name, call in (("forward_vertices", lambda: ops.forward_vertices_raw(slab)),
                       ("marching_cubes", lambda: ops.marching_cubes_raw(slab)),
                       ("keep_largest_raw", lambda: ops.keep_largest_raw(slab))):
        with pytest.raises(ValueError, match="%s wants a cubic volume" % name):
            call()
    with pytest.raises(ValueError, match="faces must be a contiguous .* int32"):
        ops.mesh_normals_raw(v, f.long(), c)
    with pytest.raises(ValueError, match="counts must be a contiguous int32"):
        ops.mesh_normals_raw(v, f, c.long())
    with pytest.raises(ValueError, match="counts must be a contiguous int32"):
        ops.mesh_points_raw(v, c.long())
    with pytest.raises(ValueError, match="verts must be a contiguous .* float32"):
        ops.mesh_points_raw(v.double(), c)
    with pytest.raises(ValueError, match="normals mode"):
        ops.mesh_normals_raw(v, f, c, mode="area")
    for bad in (torch.zeros(5, 3), torch.zeros(6, 3, dtype=torch.float64), torch.zeros(3, 6).t(), torch.zeros(1, 6, 3)):
        with pytest.raises(ValueError, match="mesh_normals_raw: out must be float32"):
            ops.mesh_normals_raw(v, f, c, out=bad)
    cube = torch.zeros(5, 5, 5)
    for bad in (torch.zeros(5, 5, 4), torch.zeros(5, 5, 5, dtype=torch.float64), torch.zeros(125)):
        with pytest.raises(ValueError, match="keep_largest_raw: out.* must be float32"):
            ops.keep_largest_raw(cube, out=bad)
    for kw in (dict(connectivity=18), dict(fill=0.75), dict(fill=float("nan"))):
        with pytest.raises(ValueError, match="keep_largest_raw: (connectivity|fill)"):
            ops.keep_largest_raw(cube, **kw)


def test_frame_chunks_cover_the_frames_in_order():
    from monoport_amd import ops
    most = ops.MAX_FRAMES
    for n in (1, most, most + 1, 2 * most + 3):
        chunks = list(ops._frame_chunks(n))
        assert chunks[0][0] == 0 and chunks[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))  # contiguous, in order
        assert all(1 <= f1 - f0 <= most for f0, f1 in chunks)
        assert [f for f0, f1 in chunks for f in range(f0, f1)] == list(range(n))
        assert len(chunks) == -(-n // most)
    assert list(ops._frame_chunks(0)) == []
