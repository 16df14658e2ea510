"""``samples`` without a GPU: the raster record and its fine form, the slots' picture option, and the refusals of the
render calls, all of which come before anything is allocated or enqueued."""
import inspect

import numpy as np
import pytest

from test_views_slot_cpu import _net

torch = pytest.importorskip("torch")
MESH = {"normals": "accumulate", "colors": False}


def test_raster_carries_samples_beside_its_six_fields():
    from monoport_amd import ops
    plain = ops.raster("who", (24, 40))
    assert plain.samples == 1 and ops.fine_raster(plain) is plain
    ras = ops.raster("who", (24, 40), "perspective", "min", 0.25, 2.0, True, 3)
    assert ras.samples == 3 and isinstance(ras, ops.Raster) and len(ras) == 6
    assert ras == ((24, 40), "perspective", "min", 0.25, 2.0, True)  # what a pass reads
    fine = ops.fine_raster(ras)
    assert isinstance(fine, ops.Raster) and fine.samples == 1 and fine.res == (72, 120)
    assert fine[1:] == ras[1:]  # the same camera model, plane and background
    assert ras._replace(near=3.0).samples == 3 and ras._replace(near=3.0).near == 3.0
    assert "samples=3" in repr(ras)
    for samples in (0, 5, -1, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="who: samples must be an int in 1..4"):
            ops.raster("who", 8, samples=samples)
    assert ops.raster("who", 1024, samples=4).samples == 4 and ops.raster("who", (2048, 7), samples=2).samples == 2
    for res, samples in ((1025, 4), ((8, 1366), 3), ((2049, 8), 2)):
        with pytest.raises(ValueError, match="who: samples = %d .* outside 1..4096" % samples):
            ops.raster("who", res, samples=samples)
    with pytest.raises(ValueError, match="image size"):  # the size itself is refused first
        ops.raster("who", 4097, samples=2)


def test_picture_option():
    from monoport_amd import pipeline
    from monoport_amd.pipeline import PICTURE_KEYS, PICTURE_OPTION_KEYS, PictureOptions, _picture_options
    from monoport_amd.recon import mesh_options
    normals = mesh_options("accumulate")
    assert PICTURE_OPTION_KEYS == PICTURE_KEYS + ("samples",)
    absent = _picture_options({}, normals)
    assert absent.samples == 1 and absent.raster.samples == 1
    got = _picture_options({"samples": 2, "res": (40, 24)}, normals)
    assert isinstance(got, PictureOptions) and got.samples == 2 and got.res == (40, 24)
    assert got.raster.samples == 2 and got.raster.res == (40, 24)
    assert got == _picture_options({"res": (40, 24)}, normals)  # the tuple: what one pass at ``res`` is asked for
    for samples in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="samples must be"):
            pipeline.FrameSlot(_net("G", 1), "cpu", mesh=MESH, pictures={"samples": samples})
    with pytest.raises(ValueError, match="outside 1..4096"):
        pipeline.FrameSlot(_net("G", 1), "cpu", mesh=MESH, pictures={"samples": 4, "res": 1025})
    with pytest.raises(ValueError, match="outside 1..4096"):  # the shared option path of the multi-view slots
        pipeline.ViewsSlot(_net("G", 2), "cpu", mesh=MESH, pictures={"samples": 2, "res": (16, 2049)})
    with pytest.raises(ValueError, match="unknown keys \\['sample'\\]"):
        pipeline.FrameSlot(_net("G", 1), "cpu", mesh=MESH, pictures={"sample": 2})


def test_render_calls_take_the_keyword_and_refuse_before_a_device_is_touched():
    from monoport_amd import recon
    for fn in (recon.render_mesh, recon.render_mesh_many, recon.render_scene, recon.render_mesh_many_in_scene):
        assert inspect.signature(fn).parameters["samples"].default == 1
    assert recon.ResolvedPicture._fields == ("image", "depth", "face", "mask", "coverage")
    cam = np.eye(4, dtype=np.float32)
    mesh = recon.Mesh(torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32), None, torch.zeros(3, 3))
    for samples in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="samples must be"):
            recon.render_mesh(mesh, cam, 8, samples=samples)
        with pytest.raises(ValueError, match="samples must be"):
            recon.render_mesh(None, cam, 8, samples=samples)
        with pytest.raises(ValueError, match="samples must be"):
            recon.render_mesh_many([mesh], cam, 8, samples=samples)
    with pytest.raises(ValueError, match="outside 1..4096"):
        recon.render_mesh(mesh, cam, (8, 1025), samples=4)
    with pytest.raises(ValueError, match="outside 1..4096"):
        recon.render_mesh_many([None], cam, 2049, samples=2)
    assert recon.render_mesh(None, cam, 8, samples=2) is None
    assert recon.render_mesh_many([None, None], cam, 8, samples=3) == [None, None]
    # the generic call and the raw wrapper refuse on the host too
    depth, face = torch.zeros(4, 6), torch.zeros((4, 6), dtype=torch.int32)
    for samples in (1, 5, 2.0):
        with pytest.raises(ValueError, match="samples must be an int in 2..4"):
            recon.resolve_picture((None, depth, face), samples)
    with pytest.raises(ValueError, match="with s = 4"):
        recon.resolve_picture((None, depth, face), 4)
    with pytest.raises(ValueError, match="MeshRender"):
        recon.resolve_picture((None, depth), 2)
