"""mp_mesh_atlas / mp_mesh_atlas_batch (csrc/atlas.hip) and their ops wrappers on the GPU: face ids, positions and info
equal the numpy restatement (tests/atlas_ref.py) BIT FOR BIT on the cases of tests/atlas_cases.py -- hand-made and
marching-cubes meshes, odd and even face counts, an atlas exactly full and one face short of room, empty meshes, counts
above the capacities, NaN / inf vertices, out-of-range indices, a cell that does not divide the side --, whatever the
output buffers held before, batched as alone, in every run; every refusal launches nothing.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

import atlas_cases as cases
import atlas_ref as ref
import glb_cases

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
OK, ARG, UNSUPPORTED = 0, -1, -3  # MP_OK, MP_ERR_ARG, MP_ERR_UNSUPPORTED (include/monoport_hip.h)
F = np.float32


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


def on_device(c):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    return t(c.verts), t(c.faces), torch.tensor(c.counts, dtype=torch.int32).to(DEV)


def dirty(c, byte, n=None):
    """Output buffers of a case (of n frames) with every byte set to ``byte``."""
    a, lead = c.size, () if n is None else (n,)
    fill = lambda shape, dtype: torch.full(shape, byte, dtype=torch.uint8, device=DEV).view(dtype)  # noqa: E731
    return (fill(lead + (a, a * 4), torch.int32), fill(lead + (a, a, 12), torch.float32), fill(lead + (8,), torch.int32))


def bits(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(got, want, what):
    for name, g, w in zip(("face_id", "position", "info"), got, want):
        g, w = bits(g), bits(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            where = np.argwhere(g != w)
            raise AssertionError("%s: %s differs at %d places, first %s" % (what, name, len(where), where[0]))


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c.name)
def test_atlas_equals_the_restatement(ops, case):
    v, f, n = on_device(case)
    want = cases.restated(case)
    got = ops.mesh_atlas_raw(v, f, n, case.size, case.cell)
    torch.cuda.synchronize()
    same(got, want, case.name)
    assert tuple(got[0].shape) == (case.size, case.size) and tuple(got[1].shape) == (case.size, case.size, 3)


def test_full_and_one_too_many(ops):
    """nf = 2 G^2 exactly fills the atlas; one face more is reported and laid out nowhere."""
    for size, cell in ((64, 8), (128, 64)):
        room = ref.capacity(size, cell)
        full, over = cases.full(size, cell, 0), cases.full(size, cell, 1)
        a = ops.mesh_atlas_raw(*on_device(full), size, cell)
        b = ops.mesh_atlas_raw(*on_device(over), size, cell)
        torch.cuda.synchronize()
        assert a[2].tolist() == [room, room] and b[2].tolist() == [room, room + 1]
        assert int(a[0].max()) == int(b[0].max()) == room - 1
        same(b, cases.restated(over), "one too many")


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_dirty_outputs(ops, byte):
    """The call writes every texel: the same bits whatever the buffers held (it uses no scratch arena)."""
    for case in (cases.hand_made(3, 64, 5), cases.sphere_case(17, 64, 4), glb_case(13), glb_case(3, 128, 5)):
        out = dirty(case, byte)
        got = ops.mesh_atlas_raw(*on_device(case), case.size, case.cell, out=out)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == out[0].data_ptr()
        same(got, cases.restated(case), "%s over 0x%02X" % (case.name, byte))


def glb_case(k, size=64, cell=8):
    return cases._from_glb(glb_cases.small_cases()[k], size, cell)


def batch_of_three():
    """Three meshes of one capacity with a gated-off {0, 0} frame in the middle."""
    return [cases._from_glb(glb_cases.random_mesh("atlas_batch_%d" % k, 90, 61, 50 + k, glb_cases.SKEW, counts=n), 64, 8)
            for k, n in enumerate(((90, 61), (0, 0), (40, 22)))]


def test_batched_equals_per_frame_and_runs_repeat(ops):
    frames = batch_of_three()
    parts = [on_device(c) for c in frames]
    runs = []
    for byte in (0x00, 0xA5):
        got = ops.mesh_atlas_raw_batch(*[[p[k] for p in parts] for k in range(3)], 64, 8, 0.25, out=dirty(frames[0], byte, 3))
        torch.cuda.synchronize()
        runs.append(got)
    for i, c in enumerate(frames):
        want = cases.restated(c, 0.25)
        alone = ops.mesh_atlas_raw(*parts[i], 64, 8, 0.25)
        torch.cuda.synchronize()
        for got in (runs[0][i], runs[1][i], alone):
            same(got, want, "frame %d" % i)
    assert runs[0][1][2].tolist() == [0, 0] and int(runs[0][1][0].max()) == -1
    fresh = ops.mesh_atlas_raw_batch(*[[p[k] for p in parts] for k in range(3)], 64, 8, 0.25)
    torch.cuda.synchronize()
    for i in range(3):
        same(fresh[i], runs[0][i], "fresh buffers %d" % i)


class Env:
    """A well-formed call of mp_mesh_atlas_batch on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        self.frames = batch_of_three()[::2]
        self.t = [on_device(c) for c in self.frames]
        self.out = [torch.full((2, 64, 64), -7, dtype=torch.int32, device=DEV),
                    torch.full((2, 64, 64, 3), -7.0, dtype=torch.float32, device=DEV),
                    torch.full((2, 2), -7, dtype=torch.int32, device=DEV)]
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def ptrs(self, k, shift=None):
        p = [t[k].data_ptr() for t in self.t]
        if shift is not None:
            p[1] = shift(p[1])
        return (ctypes.c_void_p * 2)(*p)

    def outs(self, k, shift=None):
        p = [self.out[k][0].data_ptr(), self.out[k][1].data_ptr()]
        if shift is not None:
            p[1] = shift(p[1])
        return (ctypes.c_void_p * 2)(*p)

    def call(self, **k):
        a = dict(n=2, verts=self.ptrs(0), max_v=90, faces=self.ptrs(1), max_f=61, counts=self.ptrs(2), size=64, cell=8,
                 background=0.5, face_id=self.outs(0), position=self.outs(1), info=self.outs(2))
        a.update(k)
        rc = self.lib.mp_mesh_atlas_batch(self.ctx.handle, a["n"], a["verts"], a["max_v"], a["faces"], a["max_f"],
                                          a["counts"], a["size"], a["cell"], a["background"], a["face_id"], a["position"],
                                          a["info"], self.stream)
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    nan, inf = float("nan"), float("inf")
    null_second = lambda p: None  # noqa: E731
    v1, f1 = env.t[1][0].data_ptr(), env.t[1][1].data_ptr()
    face0 = env.out[0][0].data_ptr()
    refused = [
        (dict(size=32), ARG, "atlas_size"), (dict(size=8192), ARG, "atlas_size"), (dict(size=96), ARG, "atlas_size"),
        (dict(size=0), ARG, "atlas_size"), (dict(size=-64), ARG, "atlas_size"),
        (dict(cell=3), ARG, "cell"), (dict(cell=65), ARG, "cell"), (dict(cell=0), ARG, "cell"),
        (dict(n=0), ARG, "frame"), (dict(n=-1), ARG, "frame"), (dict(n=33), ARG, "frame"),
        (dict(verts=None), ARG, "bad argument"), (dict(faces=None), ARG, "bad argument"),
        (dict(counts=None), ARG, "bad argument"), (dict(face_id=None), ARG, "bad argument"),
        (dict(position=None), ARG, "bad argument"), (dict(info=None), ARG, "bad argument"),
        (dict(max_v=-1), ARG, "bad argument"), (dict(max_f=-1), ARG, "bad argument"),
        (dict(background=nan), ARG, "non-finite"), (dict(background=inf), ARG, "non-finite"),
        (dict(background=-inf), ARG, "non-finite"),
        (dict(max_v=2 ** 31 // 3 + 1), UNSUPPORTED, "2^31"), (dict(max_f=2 ** 31 // 3 + 1), UNSUPPORTED, "2^31"),
        (dict(verts=env.ptrs(0, null_second)), ARG, "null buffer for frame 1"),
        (dict(counts=env.ptrs(2, null_second)), ARG, "null buffer for frame 1"),
        (dict(face_id=env.outs(0, null_second)), ARG, "null buffer for frame 1"),
        (dict(position=env.outs(1, null_second)), ARG, "null buffer for frame 1"),
        (dict(info=env.outs(2, null_second)), ARG, "null buffer for frame 1"),
        (dict(verts=env.ptrs(0, lambda p: p + 2)), ARG, "misaligned buffer for frame 1"),
        (dict(faces=env.ptrs(1, lambda p: p + 1)), ARG, "misaligned buffer for frame 1"),
        (dict(face_id=env.outs(0, lambda p: p + 2)), ARG, "misaligned buffer for frame 1"),
        (dict(position=env.outs(1, lambda p: p + 3)), ARG, "misaligned buffer for frame 1"),
        (dict(info=env.outs(2, lambda p: p + 1)), ARG, "misaligned buffer for frame 1"),
        (dict(face_id=env.outs(0, lambda p: v1)), ARG, "aliases an input"),
        (dict(position=env.outs(1, lambda p: f1 + 4)), ARG, "aliases an input"),
        (dict(info=env.outs(2, lambda p: env.t[0][2].data_ptr())), ARG, "aliases an input"),
        (dict(position=env.outs(1, lambda p: v1 - 64 * 64 * 12 + 4)), ARG, "aliases an input"),
        (dict(face_id=env.outs(0, lambda p: face0 + 4 * 64 * 64 - 4)), ARG, "aliases an output"),
        (dict(position=env.outs(1, lambda p: face0)), ARG, "aliases an output"),
        (dict(info=env.outs(2, lambda p: env.out[1][0].data_ptr() + 8)), ARG, "aliases an output"),
    ]
    for changed, code, word in refused:
        rc, msg = env.call(**changed)
        assert rc == code and msg.startswith("mp_mesh_atlas_batch:") and word in msg, (changed, rc, msg)
    one = env.t[0]
    rc = env.lib.mp_mesh_atlas(env.ctx.handle, one[0].data_ptr(), 90, one[1].data_ptr(), 61, one[2].data_ptr(), 100, 8, 0.5,
                               env.out[0].data_ptr(), env.out[1].data_ptr(), env.out[2].data_ptr(), env.stream)
    msg = env.lib.mp_last_error(env.ctx.handle).decode()
    assert rc == ARG and msg.startswith("mp_mesh_atlas:") and "atlas_size" in msg
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in env.out)  # nothing was launched
    # the context is still usable, and capacities of 0 need no buffers
    assert env.call()[0] == OK
    torch.cuda.synchronize()
    for i, c in enumerate(env.frames):
        same([o[i] for o in env.out], cases.restated(c), "after the refusals %d" % i)
    for k in (dict(max_v=0, verts=None), dict(max_f=0, faces=None)):
        assert env.call(**k)[0] == OK
        torch.cuda.synchronize()
        assert bool((env.out[0] == -1).all()) and bool((env.out[1] == 0.5).all()) and env.out[2].tolist() == [[0, 0]] * 2


def test_wrapper_refusals(ops):
    c = cases.hand_made(3)
    v, f, n = on_device(c)
    for bad in (dict(size=100), dict(size=32), dict(size=64.0), dict(cell=3), dict(cell=65), dict(cell=True),
                dict(background=np.nan), dict(background="grey"),
                dict(out=(torch.zeros((32, 32), dtype=torch.int32, device=DEV),) * 3)):
        kw = dict(size=64, cell=8)
        kw.update(bad)
        with pytest.raises(ValueError, match="mesh_atlas_raw"):
            ops.mesh_atlas_raw(v, f, n, **kw)
    with pytest.raises(ValueError):
        ops.mesh_atlas_raw(v.double(), f, n, 64, 8)
    with pytest.raises(ValueError, match="one capacity"):
        ops.mesh_atlas_raw_batch([v, v[:-1]], [f, f], [n, n], 64, 8)
    assert ops.atlas_faces(128, 5) == 2 * 25 * 25 and ops.atlas_faces(4096, 4) == 2 * 1024 ** 2
