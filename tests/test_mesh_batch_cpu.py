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
    from monoport_amd import pipeline, recon
    assert tuple(pipeline._mesh_options({}, 0.5, True)[:3]) == ("accumulate", 0.5, True)
    assert tuple(pipeline._mesh_options({"normals": None, "level": 0.25}, 0.5, False)[:3]) == (None, 0.25, False)
    assert tuple(pipeline._mesh_options({"normals": "reference", "colors": False}, 0.4, True)[:3]) == ("reference", 0.4, False)

    class Options:
        normals = "reference"

    assert tuple(pipeline._mesh_options(Options(), 0.5, False)[:3]) == ("reference", 0.5, False)
    for bad in ({"normals": "area"}, {"colours": True}, {"colors": True}):
        with pytest.raises(ValueError):
            pipeline._mesh_options(bad, 0.5, False)
    assert 1 <= pipeline.MESH_BATCH <= pipeline.MAX_RECON_BATCH

    # clean, simplify, smooth: fields of the same record, from a dict and from an object with attributes alike
    def as_object(options):
        return type("Options", (), dict(options))()

    three = dict(iterations=3, lam=0.5, mu=-0.53, pin_border=True)
    other = dict(iterations=2, lam=0.3, mu=-0.31, pin_border=False)
    for form in (dict, as_object):
        opts = pipeline._mesh_options(form({}), 0.5, True)
        assert isinstance(opts, recon.MeshOptions) and opts._fields[3:] == ("clean", "simplify", "smooth")
        assert opts.clean is None and opts.simplify is None and opts.smooth is None
        for key, value, want in (("clean", 6, 6), ("clean", 26, 26), ("simplify", 16, 16), ("simplify", 1, 1),
                                 ("simplify", 512, 512), ("smooth", 3, three), ("smooth", {"iterations": 3}, three),
                                 ("smooth", other, other)):
            opts = pipeline._mesh_options(form({key: value}), 0.5, True)
            assert getattr(opts, key) == want, (key, value)
            assert opts._replace(**{key: None}) == pipeline._mesh_options(form({}), 0.5, True), (key, value)
        assert pipeline._mesh_options(form({"clean": 6, "level": 0.25}), 0.5, False) == recon.MeshOptions(
            "accumulate", 0.25, False, 6, None, None)
        with pytest.raises(ValueError, match="clean must be None or one of"):
            pipeline._mesh_options(form({"clean": 7}), 0.5, True)
        with pytest.raises(ValueError, match="clean .* level > 0"):
            pipeline._mesh_options(form({"clean": 6, "level": 0}), 0.5, True)
        for bad in (0, 513, 16.0):
            with pytest.raises(ValueError, match="simplify: cells per axis"):
                pipeline._mesh_options(form({"simplify": bad}), 0.5, True)
        for bad in (0, 65, -1, 3.0, "3", True, {}, {"lam": 0.5}, {"iterations": 3, "lambda": 0.5},
                    {"iterations": 3, "mu": float("nan")}, {"iterations": 3, "pin_border": "yes"}):
            with pytest.raises(ValueError, match="smooth: "):
                pipeline._mesh_options(form({"smooth": bad}), 0.5, True)
    with pytest.raises(ValueError, match="normals"):
        pipeline._mesh_options(as_object({"normals": "area"}), 0.5, True)
    with pytest.raises(ValueError, match="colors need netC"):
        pipeline._mesh_options(as_object({"colors": True}), 0.5, False)
