"""What FrameSlot / ViewsSlot(pictures=...) accept and refuse, without a GPU: the options are validated before anything
is allocated, so device "cpu" gets as far as the refusal (tests/test_views_slot_cpu.py's way)."""
import math

import pytest

from test_views_slot_cpu import _net

torch = pytest.importorskip("torch")
MESH = {"normals": "accumulate", "colors": False}


def refused(match, pictures, mesh=MESH, netc=None, exc=ValueError):
    from monoport_amd import pipeline
    with pytest.raises(exc, match=match):
        pipeline.FrameSlot(_net("G", 1), "cpu", netC=netc, mesh=mesh, pictures=pictures)


def test_picture_options_are_validated_before_any_allocation():
    refused("unknown keys \\['size'\\]", {"size": 64})
    refused("a dict", ["views"])
    refused("needs mesh", {"views": 1}, mesh=None)
    for views in (0, -1, 1.5, "2", True):
        refused("views must be", {"views": views})
    for res in (0, 4097, (16, 0), (5000, 16)):
        refused("image size", {"res": res})
    refused("shade must be", {"shade": "depth"})
    refused("normals=None", {"shade": "normals"}, mesh={"normals": None, "colors": False})
    refused("shade='colors' needs", {"shade": "colors"})
    refused("colors need netC", {"shade": "colors"}, mesh={"normals": "accumulate", "colors": True})
    refused("projection", {"projection": "fisheye"})
    refused("nearest", {"nearest": "closest"})
    refused("perspective_correct needs near", {"projection": "perspective", "perspective_correct": True})
    refused("perspective cameras only", {"near": 0.5})
    refused("perspective cameras only", {"near": 0.5, "projection": "orthogonal", "perspective_correct": True})
    for near in (0.0, -2.0, math.inf, math.nan):
        refused("near must be", {"near": near, "projection": "perspective"})


def test_views_slot_inherits_the_option():
    from monoport_amd import pipeline
    with pytest.raises(ValueError, match="unknown keys"):
        pipeline.ViewsSlot(_net("G", 2), "cpu", mesh={"normals": "accumulate"}, pictures={"cameras": 2})
    with pytest.raises(ValueError, match="needs mesh"):
        pipeline.ViewsSlot(_net("G", 2), "cpu", pictures={"views": 2})
    with pytest.raises(ValueError, match="shade='colors' needs"):
        pipeline.ViewsSlot(_net("G", 2), "cpu", mesh={"normals": "accumulate"}, pictures={"shade": "colors"})
    with pytest.raises(ValueError, match="single-view"):  # the slot class's own refusals still come first
        pipeline.ViewsSlot(_net("G", 1), "cpu", pictures={"size": 3})


def test_picture_options_record():
    from monoport_amd.pipeline import PICTURE_KEYS, PictureOptions, _picture_options
    from monoport_amd.recon import mesh_options
    normals, colours = mesh_options("accumulate"), mesh_options(None, colors=True)
    assert PictureOptions._fields == PICTURE_KEYS
    assert _picture_options({}, normals) == PictureOptions(1, (257, 257), "normals", "orthogonal", "max", None, False, 1.0)
    assert _picture_options({}, colours).shade == "colors"
    assert _picture_options({}, mesh_options(None)).shade is None
    got = _picture_options(dict(views=4, res=(40, 24), shade=None, projection="perspective", nearest="min", near=2,
                                perspective_correct=1, background=0), colours)
    assert got == PictureOptions(4, (40, 24), None, "perspective", "min", 2.0, True, 0.0)
    assert isinstance(got.near, float) and got.perspective_correct is True


def test_raster_record():
    """ops.Raster: the six rasteriser arguments as one record, made by ops.raster with the checks and texts of the
    render calls, and what PictureOptions.raster hands to the recon bodies."""
    from monoport_amd import ops
    from monoport_amd.pipeline import _picture_options
    from monoport_amd.recon import mesh_options
    who = "FrameSlot(pictures=...)"
    assert ops.Raster._fields == ("res", "projection", "nearest", "background", "near", "perspective_correct")
    colours = mesh_options(None, colors=True)
    got = _picture_options({}, colours).raster
    assert isinstance(got, ops.Raster) and got == ops.raster(who, 257)
    assert got == ((257, 257), "orthogonal", "max", 1.0, None, False)
    got = _picture_options(dict(views=4, res=(40, 24), shade=None, projection="perspective", nearest="min", near=2,
                                perspective_correct=1, background=0), colours).raster
    assert got == ops.raster(who, (40, 24), "perspective", "min", 0, 2, 1)
    assert got == ((40, 24), "perspective", "min", 0.0, 2.0, True)
    assert isinstance(got.near, float) and isinstance(got.background, float) and got.perspective_correct is True
    for res in (0, 4097, (16, 0), (5000, 16)):
        with pytest.raises(ValueError, match="who: image size"):
            ops.raster("who", res)
    with pytest.raises(ValueError, match="projection must be one of"):
        ops.raster("who", 8, "fisheye")
    with pytest.raises(ValueError, match="nearest must be one of"):
        ops.raster("who", 8, nearest="closest")
    with pytest.raises(ValueError, match="who: near clips perspective cameras only"):
        ops.raster("who", 8, near=0.5)
    with pytest.raises(ValueError, match="who: perspective_correct needs near"):
        ops.raster("who", 8, "perspective", perspective_correct=True)
    for near in (0.0, -2.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="who: near must be"):
            ops.raster("who", 8, "perspective", near=near)
    assert ops.raster("who", 8, "perspective", near=3) == ((8, 8), "perspective", "max", 1.0, 3.0, False)


def test_render_keywords_are_refused_without_a_device():
    import os
    import re
    from monoport_amd import _lib, ops, recon
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "monoport_hip.h")).read()
    assert int(re.search(r"\bMP_RENDER_PERSPECTIVE_CORRECT\s*=\s*(\d+)", header).group(1)) == _lib.RENDER_PERSPECTIVE_CORRECT
    with pytest.raises(ValueError, match="perspective_correct needs near"):
        recon.render_mesh_many([None], torch.eye(4), projection="perspective", perspective_correct=True)
    with pytest.raises(ValueError, match="perspective cameras only"):
        recon.render_mesh_many([None], torch.eye(4), near=1.0)
    assert recon.render_mesh_many([None], torch.eye(4), projection="perspective", near=1.0) == [None]
    assert ops._render_clip("x", "perspective", None, False) is None
    assert ops._render_clip("x", 1, 0.25, True) == (0.25, 1) and ops._render_clip("x", "perspective", 3, False) == (3.0, 0)
