"""The argument checks the query / reconstruction wrappers of monoport_amd.ops share, on CPU tensors (they need no
context), the MAX_FRAMES constant against the kernels' kMaxFrames, and that importing ops does not load the library."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_max_frames_matches_the_kernels():
    from monoport_amd import _lib, ops
    src = open(os.path.join(ROOT, "monoport_amd", "csrc", "mp_internal.h")).read()
    m = re.search(r"constexpr int kMaxFrames = (\d+);", src)
    assert m and int(m.group(1)) == _lib.MAX_FRAMES == ops.MAX_FRAMES == 32
    assert _lib.load().mp_max_frames() == _lib.MAX_FRAMES


def test_scratch_fill_refuses_without_a_context():
    """The test hook mp_scratch_fill returns MP_ERR_ARG for a NULL context before it looks at anything else (no
    device is touched: this passes on a machine without one), and ops.scratch_fill names its roles."""
    from monoport_amd import _lib, ops
    lib = _lib.load()
    block = ctypes.c_int64(-7)
    for nbytes, value in ((1024, 0), (0, 255), (-1, 0), (1024, 256)):
        assert lib.mp_scratch_fill(None, nbytes, value, ctypes.byref(block), None) == -1  # MP_ERR_ARG
        assert lib.mp_scratch_fill(None, nbytes, value, None, None) == -1
    assert block.value == -7
    with pytest.raises(ValueError, match="role"):
        ops.scratch_fill("cuda:0", 16, 0, role="mesh")


def test_importing_ops_does_not_load_the_library(tmp_path):
    """MONOPORT_HIP_LIB is read when _lib is imported: with a missing file there, the import still succeeds and only
    loading raises."""
    env = dict(os.environ, MONOPORT_HIP_LIB=str(tmp_path / "missing.so"), PYTHONPATH=ROOT)
    code = ("import monoport_amd.ops as ops, monoport_amd._lib as L\n"
            "assert L._lib is None and ops.MAX_FRAMES == 32\n"
            "try:\n    L.load()\nexcept RuntimeError as e:\n    print('refused:', 'is missing' in str(e))\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "refused: True" in r.stdout


def test_float3():
    from monoport_amd.ops import _float3
    for v in ([1, 2.5, -3], np.array([[1, 2.5, -3]]), torch.tensor([1, 2.5, -3])):
        a = _float3(v)
        assert isinstance(a, ctypes.c_float * 3) and list(a) == [1.0, 2.5, -3.0]
    with pytest.raises(ValueError):
        _float3([1, 2])


def test_ptr_array():
    from monoport_amd.ops import _ptr_array
    t = torch.zeros(3, 5)
    a = _ptr_array([t, None, t[1]])
    assert len(a) == 3 and a[0] == t.data_ptr() and a[1] is None and a[2] == t.data_ptr() + 20
    assert list(_ptr_array(t)) == [t.data_ptr() + 20 * i for i in range(3)]  # a tensor: one entry per row


def test_cubic_volume():
    from monoport_amd.ops import _cubic_volume
    v = torch.arange(27, dtype=torch.float64).reshape(1, 1, 3, 3, 3)
    out = _cubic_volume(v, "f")
    assert out.shape == (3, 3, 3) and out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out, v[0, 0].float())
    assert _cubic_volume(out.permute(2, 1, 0), "f").is_contiguous()
    for bad in (torch.zeros(3, 3, 4), torch.zeros(3, 3), torch.zeros(2, 3, 3, 3)[:, :, :, :2]):
        with pytest.raises(ValueError, match="f wants a cubic volume"):
            _cubic_volume(bad, "f")


def test_calib_list():
    from monoport_amd.ops import _calib_list
    c = torch.eye(4)[None].repeat(3, 1, 1)
    got = _calib_list(c, 3, "f")
    assert len(got) == 3 and all(torch.equal(g, torch.eye(4)) for g in got)
    lst = [torch.eye(4)[None], torch.eye(4)[:3]]
    assert _calib_list(lst, 2, "f") is lst
    for bad, n in ((c, 2), (lst, 3), ([], 1)):
        with pytest.raises(ValueError, match="f: %d maps, %d calibrations" % (n, len(bad))):
            _calib_list(bad, n, "f")


def test_maps():
    from monoport_amd.ops import _maps
    m = [torch.zeros(4, 6, 8) for _ in range(2)]
    assert _maps("f", m) == (4, 6, 8, torch.device("cpu"))
    for bad in ([m[0], torch.zeros(4, 6, 16)], [m[0], torch.zeros(6, 4, 8).transpose(0, 1)], [m[0], m[1].double()],
                [m[0].half(), m[1]]):
        with pytest.raises(ValueError, match=r"f: the maps must be contiguous float32 \[4,6,8\]"):
            _maps("f", bad)
    for bad in ([], [torch.zeros(4, 6)]):
        with pytest.raises(ValueError, match="f: wants a non-empty list"):
            _maps("f", bad)


def test_out_rows():
    from monoport_amd.ops import _out_rows
    _out_rows("f", torch.zeros(2, 3, 5), 2, 3, 5)
    _out_rows("f", torch.zeros(4, 3, 5)[::2], 2, 3, 5)            # rows contiguous, the stack of them not
    _out_rows("f", torch.zeros(2, 3, 0), 2, 3, 0)
    for bad in (torch.zeros(2, 3, 4), torch.zeros(2, 1, 5), torch.zeros(2, 3, 5).double(),
                torch.zeros(2, 5, 3).transpose(1, 2)):
        with pytest.raises(ValueError, match="f: out must be float32"):
            _out_rows("f", bad, 2, 3, 5)


def test_check_count_and_early_arg_without_flags():
    from monoport_amd.ops import _check_count, _early_arg
    _check_count("f", "frames", 1, 32)
    _check_count("f", "frames", 32, 32)
    for n in (0, 33):
        with pytest.raises(ValueError, match="f: 1..32 frames per call, got %d" % n):
            _check_count("f", "frames", n, 32)
    assert _early_arg("f", None, 3, None, 17) is None


def test_bindings_carry_what_the_engine_asks():
    """Seg3dLossless drives a binding through trust_key / check_view / recon / batchable alone."""
    from monoport_amd.modeling.MonoPortNet import QueryBinding, ViewsBinding

    class Head:
        precision = "f32"

    head = Head()
    q = QueryBinding(None, head, "map", "calib", 2, projection=1)
    assert q.batchable and q.trust_key(5) == (id(head), "f32", 2.0, 1)
    q.check_view(5)
    v = ViewsBinding(None, head, ["a", "b"], "calibs", 2, projection=0)
    assert not v.batchable and v.trust_key(1) == (id(head), "f32", 2.0, 2, 1, 0)
    v.check_view(1)
    with pytest.raises(ValueError, match="view=2"):
        v.check_view(2)
