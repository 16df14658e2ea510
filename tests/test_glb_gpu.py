"""mp_mesh_glb / mp_mesh_glb_batch (csrc/glb.hip) and their ops wrappers on the GPU: every file and every info row equals
the numpy restatement (tests/glb_ref.py) BYTE FOR BYTE on the cases of tests/glb_cases.py, with every attribute set and
both colour layouts, on a fresh and on a dirty scratch arena, in every run, batched as alone; a capacity one byte short
reports the size and writes nothing; every refusal launches nothing.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import glb_cases as cases
import glb_ref as ref
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, -1, -3  # MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED (include/monoport_hip.h)
F = np.float32
SENTINEL = 0xA5
SMALL = cases.small_cases()


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


def on_device(c, normals=True, colors=True, layout="rows"):
    """(verts, faces, counts, normals or None, colours or None) of a case as device tensors."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    col = None
    if colors:
        col = t(c.colors.T) if layout == "planes" else t(c.colors)
    return (t(c.verts), t(c.faces), torch.tensor(c.counts, dtype=torch.int32).to(DEV),
            t(c.normals) if normals else None, col)


def device_file(ops, c, normals=True, colors=True, layout="rows", scale=1.0, bias=0.0, **kw):
    """mp_mesh_glb of one case -> (out [1,capacity], info [1,2]) on the host."""
    v, f, n, nrm, col = on_device(c, normals, colors, layout)
    out, info = ops.mesh_glb_raw(v, f, n, nrm, col, layout, scale, bias, c.b_min, c.b_max, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy()


def same(got, want, what):
    if got != want:
        first = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
        raise AssertionError("%s: byte %d of %d (got %d) differs" % (what, first, len(want), len(got)))


def check(ops, c, *flags, **kw):
    want = cases.restated(c, *flags)
    out, info = device_file(ops, c, *flags, **kw)
    assert tuple(info[0]) == (len(want), 0), (c.name, flags, info[0], len(want))
    same(out[0, :len(want)].tobytes(), want, "%s %s" % (c.name, flags))
    assert len(want) <= ops.glb_max_bytes(len(c.verts), len(c.faces), *flags[:2])
    return want


@pytest.mark.parametrize("flags", cases.ATTRIBUTE_SETS, ids=str)
@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_files_equal_the_restatement(ops, case, flags):
    """One triangle, odd and even face counts, more than one workgroup, vertices on / outside / far outside a skew box,
    NaN / inf / -0.0, zero-length normals, out-of-range indices, counts above the capacities, empty meshes."""
    check(ops, case, *flags)


@pytest.mark.parametrize("case", cases.index_width_cases(), ids=lambda c: c.name)
def test_index_width(ops, case):
    want = check(ops, case)
    assert ref.Glb(want).json["accessors"][-1]["componentType"] == (5123 if len(case.verts) <= 65535 else 5125)


def test_colour_layouts(ops):
    """Planes give the bytes of rows, and raw predictions as planes with (0.5, 0.5) the bytes of the finished colours as
    rows with (1, 0)."""
    c = SMALL[3]
    rows = check(ops, c, True, True, "rows")
    assert check(ops, c, True, True, "planes") == rows
    raw = ((c.colors - F(0.5)) * F(2)).astype(F)
    finished = (raw * F(0.5) + F(0.5)).astype(F)
    a, ia = device_file(ops, c._replace(colors=raw), True, True, "planes", 0.5, 0.5)
    b, ib = device_file(ops, c._replace(colors=finished), True, True, "rows", 1.0, 0.0)
    want = ref.encode(c.verts, c.faces, c.counts, c.normals, finished, "rows", 1.0, 0.0, c.b_min, c.b_max)
    assert tuple(ia[0]) == tuple(ib[0]) == (len(want), 0)
    same(a[0, :len(want)].tobytes(), want, "planes (0.5, 0.5)")
    same(b[0, :len(want)].tobytes(), want, "rows (1, 0)")


@pytest.mark.parametrize("simplify", [None, 8])
def test_marching_cubes_mesh(ops, simplify):
    """The chain's own buffers: the mesh of sphere_volume(33), plain and clustered, with its normals."""
    vol = torch.from_numpy(syn.sphere_volume(33)).to(DEV)
    verts, faces, counts = ops.marching_cubes_raw(vol)
    if simplify is not None:
        verts, faces, counts, _ = ops.mesh_simplify_raw(verts, faces, counts, simplify)
    normals = ops.mesh_normals_raw(verts, faces, counts)
    out, info = ops.mesh_glb_raw(verts, faces, counts, normals)
    torch.cuda.synchronize()
    nv, nf = counts.cpu().tolist()
    assert nv > 100 and nf > 200
    want = ref.encode(verts.cpu().numpy(), faces.cpu().numpy(), (nv, nf), normals.cpu().numpy())
    info = info.cpu().numpy()
    assert tuple(info[0]) == (len(want), 0) and len(want) == ops.glb_bytes(nv, nf, True, False)
    same(out[0, :len(want)].cpu().numpy().tobytes(), want, "sphere, simplify=%s" % simplify)
    m = ref.Glb(want).mesh()  # and the file is the mesh, within the quantisation
    assert np.array_equal(m["faces"], faces[:nf].cpu().numpy())
    assert np.abs(m["positions"] - verts[:nv].cpu().numpy().astype(np.float64)).max() <= 0.52 * 2.0 / 65535


def batch_of_three():
    """Three meshes of one capacity with a gated-off {0, 0} frame in the middle."""
    a = cases.random_mesh("batch_a", 90, 61, 21, cases.SKEW, counts=(90, 61))
    b = cases.random_mesh("batch_b", 90, 61, 22, cases.SKEW, counts=(0, 0))
    c = cases.random_mesh("batch_c", 90, 61, 23, cases.SKEW, counts=(40, 22))
    return a, b, c


def device_batch(ops, frames, **kw):
    parts = [on_device(c) for c in frames]
    out, info = ops.mesh_glb_raw_batch(*[[p[k] for p in parts] for k in range(5)], b_min=frames[0].b_min,
                                       b_max=frames[0].b_max, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), info.cpu().numpy()


def test_batched_equals_per_frame_and_runs_repeat(ops):
    frames = batch_of_three()
    runs = [device_batch(ops, frames) for _ in range(2)]
    assert np.array_equal(runs[0][1], runs[1][1])
    for i, c in enumerate(frames):
        want = cases.restated(c)
        assert tuple(runs[0][1][i]) == (len(want), 0)
        for out, _ in runs:
            same(out[i, :len(want)].tobytes(), want, "batched %d" % i)
        alone, info = device_file(ops, c)
        assert tuple(info[0]) == (len(want), 0) and alone[0, :len(want)].tobytes() == want
    assert len(cases.restated(frames[1])) == ref.MIN_BYTES


def test_capacity_exact_and_one_byte_short(ops):
    """At frame 2's exact size the call succeeds for it; at one byte less info reports the same size with the overflow
    word set, nothing of that frame is written, and the guard behind ``out`` and the rest of ``out`` keep their fill.
    The rows of an odd capacity are not dword aligned: the neighbours' bytes are the same."""
    frames = batch_of_three()
    want = [cases.restated(c) for c in frames]
    sizes = [len(b) for b in want]
    assert sizes[1] < sizes[2] < sizes[0]
    guard = 8192
    for cap in (sizes[2], sizes[2] - 1, sizes[0], sizes[0] - 1, sizes[0] + 3, ref.MIN_BYTES):
        buf = torch.full((3 * cap + guard,), SENTINEL, dtype=torch.uint8, device=DEV)
        out, info = device_batch(ops, frames, out=buf[:3 * cap].view(3, cap))
        whole = buf.cpu().numpy()
        assert (whole[3 * cap:] == SENTINEL).all()
        for i in range(3):
            fits = sizes[i] <= cap
            assert tuple(info[i]) == (sizes[i], 0 if fits else 1), (cap, i, info[i])
            if fits:
                assert out[i, :sizes[i]].tobytes() == want[i] and (out[i, sizes[i]:] == SENTINEL).all(), (cap, i)
            else:
                assert (out[i] == SENTINEL).all(), (cap, i)
    # a second call at the reported size gives the bytes a sufficient capacity gives
    out, info = device_file(ops, frames[0], capacity=sizes[0])
    assert tuple(info[0]) == (sizes[0], 0) and out[0].tobytes() == want[0]


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_dirty_arena(ops, byte):
    for c in (SMALL[0], SMALL[3], SMALL[5], SMALL[13]):
        ops.scratch_fill(DEV, 1 << 20, byte)
        check(ops, c)


def test_max_bytes(ops):
    for nv, nf in ((1, 1), (65535, 9), (65536, 9), (12 * 257 * 257, 24 * 257 * 257)):
        for flags in cases.ATTRIBUTE_SETS:
            assert ops.glb_max_bytes(nv, nf, *flags) == ops.glb_bytes(nv, nf, *flags) == ref.file_bytes(nv, nf, *flags)


class Env:
    """A well-formed call of mp_mesh_glb_batch on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        self.c = cases.random_mesh("env", 64, 32, 31)
        self.t = [on_device(self.c) for _ in range(2)]
        self.cap = 4096
        self.out = torch.full((2, self.cap), SENTINEL, dtype=torch.uint8, device=DEV)
        self.info = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def ptrs(self, k, shift=None):
        p = [t[k].data_ptr() for t in self.t]
        if shift is not None:
            p[1] = shift(p[1])
        return (ctypes.c_void_p * 2)(*p)

    def call(self, **k):
        f3 = lambda v: (ctypes.c_float * 3)(*v)  # noqa: E731
        a = dict(n=2, verts=self.ptrs(0), max_v=64, faces=self.ptrs(1), max_f=32, counts=self.ptrs(2),
                 normals=self.ptrs(3), colors=self.ptrs(4), layout=0, scale=1.0, bias=0.0, b_min=f3((-1, -1, -1)),
                 b_max=f3((1, 1, 1)), out=self.out.data_ptr(), cap=self.cap, info=self.info.data_ptr())
        a.update(k)
        rc = self.lib.mp_mesh_glb_batch(self.ctx.handle, a["n"], a["verts"], a["max_v"], a["faces"], a["max_f"],
                                        a["counts"], a["normals"], a["colors"], a["layout"], a["scale"], a["bias"],
                                        a["b_min"], a["b_max"], a["out"], a["cap"], a["info"], self.stream)
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    f3 = lambda *v: (ctypes.c_float * 3)(*v)  # noqa: E731
    nan, inf = float("nan"), float("inf")
    null_second = lambda p: None  # noqa: E731
    v0 = env.t[0][0].data_ptr()
    refused = [
        (dict(n=0), ARG, "frame"), (dict(n=-1), ARG, "frame"), (dict(n=33), ARG, "frame"),
        (dict(verts=None), ARG, "bad argument"), (dict(faces=None), ARG, "bad argument"),
        (dict(counts=None), ARG, "bad argument"), (dict(out=None), ARG, "bad argument"),
        (dict(info=None), ARG, "bad argument"), (dict(b_min=None), ARG, "bad argument"),
        (dict(b_max=None), ARG, "bad argument"), (dict(max_v=-1), ARG, "bad argument"),
        (dict(max_f=-1), ARG, "bad argument"), (dict(info=env.info.data_ptr() + 2), ARG, "bad argument"),
        (dict(verts=env.ptrs(0, null_second)), ARG, "null buffer for frame 1"),
        (dict(counts=env.ptrs(2, null_second)), ARG, "null buffer for frame 1"),
        (dict(normals=env.ptrs(3, null_second)), ARG, "null buffer for frame 1"),
        (dict(colors=env.ptrs(4, null_second)), ARG, "null buffer for frame 1"),
        (dict(verts=env.ptrs(0, lambda p: p + 2)), ARG, "misaligned buffer for frame 1"),
        (dict(faces=env.ptrs(1, lambda p: p + 1)), ARG, "misaligned buffer for frame 1"),
        (dict(counts=env.ptrs(2, lambda p: p + 2)), ARG, "misaligned buffer for frame 1"),
        (dict(normals=env.ptrs(3, lambda p: p + 3)), ARG, "misaligned buffer for frame 1"),
        (dict(colors=env.ptrs(4, lambda p: p + 2)), ARG, "misaligned buffer for frame 1"),
        (dict(out=v0), ARG, "aliases"), (dict(out=v0 - 2 * env.cap + 1), ARG, "aliases"),
        (dict(out=env.t[1][1].data_ptr() + 4), ARG, "aliases"), (dict(out=env.t[1][2].data_ptr() - 8), ARG, "aliases"),
        (dict(out=env.t[0][3].data_ptr() + 12 * 64 - 1), ARG, "aliases"), (dict(out=env.t[1][4].data_ptr()), ARG, "aliases"),
        (dict(info=v0 + 8), ARG, "aliases"), (dict(info=env.t[1][2].data_ptr()), ARG, "aliases"),
        (dict(info=env.out.data_ptr() + 4), ARG, "aliases"), (dict(out=env.info.data_ptr()), ARG, "aliases"),
        (dict(b_min=f3(nan, -1, -1)), ARG, "box"), (dict(b_max=f3(1, inf, 1)), ARG, "box"),
        (dict(b_min=f3(-1, -1, -inf)), ARG, "box"), (dict(b_min=f3(1, -1, -1)), ARG, "box"),
        (dict(b_min=f3(-1, 2, -1)), ARG, "box"), (dict(b_min=f3(0, 0, 0), b_max=f3(1, 1, 1e-42)), ARG, "too thin"),
        (dict(cap=ref.MIN_BYTES - 1), ARG, "capacity"), (dict(cap=0), ARG, "capacity"), (dict(cap=-5), ARG, "capacity"),
        (dict(cap=2 ** 31 + 1), ARG, "capacity"),
        (dict(layout=2), ARG, "color_layout"), (dict(layout=-1), ARG, "color_layout"),
        (dict(scale=nan), ARG, "non-finite"), (dict(bias=-inf), ARG, "non-finite"),
        (dict(max_v=2 ** 28), UNSUPPORTED, "2^31"), (dict(max_f=2 ** 31 // 6), UNSUPPORTED, "2^31"),
        (dict(max_v=2 ** 41), UNSUPPORTED, "2^31"),
    ]
    for changed, code, word in refused:
        rc, msg = env.call(**changed)
        assert rc == code and msg.startswith("mp_mesh_glb_batch:") and word in msg, (changed, rc, msg)
    one = env.t[0]
    rc = env.lib.mp_mesh_glb(env.ctx.handle, one[0].data_ptr(), 64, one[1].data_ptr(), 32, one[2].data_ptr(), None, None, 7,
                             1.0, 0.0, f3(-1, -1, -1), f3(1, 1, 1), env.out.data_ptr(), env.cap, env.info.data_ptr(),
                             env.stream)
    msg = env.lib.mp_last_error(env.ctx.handle).decode()
    assert rc == ARG and msg.startswith("mp_mesh_glb:") and "color_layout" in msg
    torch.cuda.synchronize()
    assert (env.out == SENTINEL).all() and (env.info == -7).all()  # nothing was launched
    # the context is still usable, and capacities of 0 need no buffers
    assert env.call()[0] == OK
    torch.cuda.synchronize()
    want = cases.restated(env.c)
    info, out = env.info.cpu().numpy(), env.out.cpu().numpy()
    for i in range(2):
        assert tuple(info[i]) == (len(want), 0) and out[i, :len(want)].tobytes() == want
    assert env.call(max_v=0, verts=None, normals=None, colors=None)[0] == OK
    assert env.call(max_f=0, faces=None)[0] == OK
    torch.cuda.synchronize()
    empty = cases.restated(cases.small_cases()[13])
    info, out = env.info.cpu().numpy(), env.out.cpu().numpy()
    for i in range(2):
        assert tuple(info[i]) == (ref.MIN_BYTES, 0) and out[i, :ref.MIN_BYTES].tobytes() == empty


def test_wrapper_refusals(ops):
    c = SMALL[1]
    v, f, n, nrm, col = on_device(c)
    for bad in (dict(color_layout="columns"), dict(color_scale=np.nan), dict(color_bias=np.inf), dict(capacity=99),
                dict(normals=nrm[:-1]), dict(colors=col.t().contiguous()), dict(colors=col.double()),
                dict(colors=col, color_layout="planes"), dict(out=torch.zeros((2, 4096), dtype=torch.uint8, device=DEV)),
                dict(info=torch.zeros((1, 2), dtype=torch.int64, device=DEV)),
                dict(out=torch.zeros((1, 4096), dtype=torch.uint8, device=DEV), capacity=4095)):
        with pytest.raises(ValueError, match="mesh_glb_raw"):
            ops.mesh_glb_raw(v, f, n, **bad)
    with pytest.raises(ValueError):
        ops.mesh_glb_raw(v.double(), f, n)
    with pytest.raises(ValueError, match="one capacity"):
        ops.mesh_glb_raw_batch([v, v[:-1]], [f, f], [n, n])
