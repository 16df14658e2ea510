"""The batched mesh chain without a GPU: what recon.reconstruct_mesh_many answers and refuses before it touches a
device, and the three batched entry points in the binding table with the argument counts the header declares."""
import os
import re

import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mp_marching_cubes_batch", "mp_mesh_normals_batch", "mp_mesh_points_batch")


def test_nothing_to_do_touches_no_device():
    from monoport_amd import recon
    assert recon.reconstruct_mesh_many([]) == []
    assert recon.reconstruct_mesh_many([None, None, None]) == [None, None, None]
    assert recon.reconstruct_mesh_many([None], normals=None) == [None]


def test_refusals_come_before_any_device_call():
    """CPU tensors: a call that reached the library would raise MonoportError (no CPU path), not ValueError."""
    from monoport_amd import recon
    from monoport_amd.modeling import PIFuNetC
    a, b = torch.zeros(5, 5, 5), torch.zeros(9, 9, 9)
    with pytest.raises(ValueError, match="one size"):
        recon.reconstruct_mesh_many([a, None, b])
    with pytest.raises(ValueError, match="normals"):
        recon.reconstruct_mesh_many([a], normals="area")
    with pytest.raises(ValueError, match="normals"):
        recon.reconstruct_mesh_many([], normals="area")
    netC = PIFuNetC().eval()
    feats = [[torch.zeros(1, 512, 128, 128)]]
    with pytest.raises(ValueError, match="2 volumes, 1 feature sets, 2 calibrations"):
        recon.reconstruct_mesh_many([a, a], netC=netC, feat_tensors_C=[feats], calib_tensors=[None, None])
    with pytest.raises(ValueError, match="2 volumes, 2 feature sets, 3 calibrations"):
        recon.reconstruct_mesh_many([a, a], netC=netC, feat_tensors_C=[feats, feats], calib_tensors=[None] * 3)
    with pytest.raises(ValueError, match="feat_tensors_C"):
        recon.reconstruct_mesh_many([a], netC=netC)


def test_batch_wrappers_check_their_lists_on_the_host():
    from monoport_amd import ops
    v, f = torch.zeros(6, 3), torch.zeros(4, 3, dtype=torch.int32)
    c = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="at least one"):
        ops.marching_cubes_raw_batch([])
    with pytest.raises(ValueError, match="cubic"):
        ops.marching_cubes_raw_batch([torch.zeros(3, 4, 5)])
    with pytest.raises(ValueError, match="one size"):
        ops.marching_cubes_raw_batch([torch.zeros(5, 5, 5), torch.zeros(9, 9, 9)])
    with pytest.raises(ValueError, match="2 volumes, 1 gates"):
        ops.marching_cubes_raw_batch([torch.zeros(5, 5, 5)] * 2, gates=[None])
    with pytest.raises(ValueError, match="int32"):
        ops.marching_cubes_raw_batch([torch.zeros(5, 5, 5)], gates=[torch.zeros(1)])
    with pytest.raises(ValueError, match="2 vertex buffers, 1 face buffers, 2 counts"):
        ops.mesh_normals_raw_batch([v, v], [f], [c, c])
    with pytest.raises(ValueError, match="one capacity"):
        ops.mesh_normals_raw_batch([v, torch.zeros(7, 3)], [f, f], [c, c])
    with pytest.raises(ValueError, match="int32"):
        ops.mesh_normals_raw_batch([v], [f.long()], [c])
    with pytest.raises(ValueError, match="normals mode"):
        ops.mesh_normals_raw_batch([v], [f], [c], mode="area")
    with pytest.raises(ValueError, match="1 vertex buffers, None face buffers, 2 counts"):
        ops.mesh_points_raw_batch([v], [c, c])
    with pytest.raises(ValueError, match="out"):
        ops.mesh_normals_raw_batch([v], [f], [c], out=torch.zeros(1, 5, 3))


def _header_arg_counts():
    text = open(os.path.join(ROOT, "include", "monoport_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    counts = {}
    for name, args in re.findall(r"\bint\s+(mp_[a-z_0-9]+)\s*\(([^;]*?)\)\s*;", text, flags=re.S):
        counts[name] = 0 if args.strip() == "void" else len(args.split(","))
    return counts


def test_new_entry_points_are_bound_as_the_header_declares():
    from monoport_amd import _lib
    declared = _header_arg_counts()
    # the parser on calls whose counts are known: mp_marching_cubes (12), mp_mesh_normals (9), mp_mesh_points (7)
    assert (declared["mp_marching_cubes"], declared["mp_mesh_normals"], declared["mp_mesh_points"]) == (12, 9, 7)
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is _lib.c_int and len(argtypes) == declared[name], name
    # n_frames and the gate array on top of the per-mesh calls
    assert declared["mp_marching_cubes_batch"] == declared["mp_marching_cubes"] + 2
    assert declared["mp_mesh_normals_batch"] == declared["mp_mesh_normals"] + 1
    assert declared["mp_mesh_points_batch"] == declared["mp_mesh_points"] + 1


def test_slot_mesh_options():
    from monoport_amd import pipeline
    assert pipeline._mesh_options({}, 0.5, True) == ("accumulate", 0.5, True)
    assert pipeline._mesh_options({"normals": None, "level": 0.25}, 0.5, False) == (None, 0.25, False)
    assert pipeline._mesh_options({"normals": "reference", "colors": False}, 0.4, True) == ("reference", 0.4, False)

    class Options:
        normals = "reference"

    assert pipeline._mesh_options(Options(), 0.5, False) == ("reference", 0.5, False)
    for bad in ({"normals": "area"}, {"colours": True}, {"colors": True}):
        with pytest.raises(ValueError):
            pipeline._mesh_options(bad, 0.5, False)
    assert 1 <= pipeline.MESH_BATCH <= pipeline.MAX_RECON_BATCH
