"""The per-frame mesh and render entries (mp_forward_vertices, mp_paint, mp_marching_cubes, mp_mesh_normals,
mp_mesh_points, mp_volume_keep_largest) through ctypes: each is its ``_batch`` entry with one frame -- the same bytes
in identically pre-filled outputs -- and shares its refusals under its own name.  Needs an MI355X."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
MP_OK, MP_ERR_ARG = 0, -1
R = 9
FILL = 0xA5  # every byte of an output before a call
F32, I32, I64 = torch.float32, torch.int32, torch.int64


class Env:
    """A 9^3 volume -- a ball of radius 3 and one detached voxel -- its visible-surface vertices and its mesh."""

    def __init__(self):
        from monoport_amd import ops
        self.ops = ops
        ctx = ops.get_context(torch.device(DEV))
        self.lib, self.h = ctx.lib, ctx.handle
        self.st = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
        z, y, x = np.mgrid[0:R, 0:R, 0:R]
        vol = ((x - 4) ** 2 + (y - 4) ** 2 + (z - 4) ** 2 <= 9).astype(np.float32)
        assert vol[0, 0, 0] == 0 and vol[1, 1, 1] == 0
        vol[0, 0, 0] = 1.0
        self.volume = torch.from_numpy(vol).to(DEV)
        self.x, self.y, _, self.norm, self.count = ops.forward_vertices_raw(self.volume, "front")
        self.verts, self.faces, self.counts = ops.marching_cubes_raw(self.volume, 0.5, [-1] * 3, [1] * 3)
        self.cap_v, self.cap_f = self.verts.shape[0], self.faces.shape[0]
        assert (self.cap_v, self.cap_f) == (12 * R * R, 24 * R * R)  # the capacities STAGES assumes
        nv, nf = self.counts.cpu().tolist()
        assert 0 < nv <= self.cap_v and 0 < nf <= self.cap_f and int(self.count.item()) > 0
        self.bmin, self.bmax = ops._float3([-1] * 3), ops._float3([1] * 3)


@pytest.fixture(scope="module")
def env():
    return Env()


# entry -> (inputs: argument name -> Env attribute; outputs: name -> (shape, dtype); args(e, p): the arguments between
# the context (and frame count) and the gate / stream, p[name] being the pointer argument of that name; has a gate)
STAGES = {
    "mp_forward_vertices": (
        dict(volume="volume"),
        dict(x=((R * R,), I64), y=((R * R,), I64), z=((R * R,), F32), norm=((R * R, 3), F32), count=((1,), I32)),
        lambda e, p: (p["volume"], R, 0, p["x"], p["y"], p["z"], p["norm"], p["count"]), False),
    "mp_paint": (
        dict(x="x", y="y", values="norm", count="count"),
        dict(image=((R, R, 3), F32)),
        lambda e, p: (p["x"], p["y"], p["values"], 0, p["count"], R * R, R, 0.5, 0.5, 0.0, 1.0, p["image"]), False),
    "mp_marching_cubes": (
        dict(volume="volume"),
        dict(verts=((12 * R * R, 3), F32), faces=((24 * R * R, 3), I32), counts=((2,), I32)),
        lambda e, p: (p["volume"], R, 0.5, e.bmin, e.bmax, p["verts"], e.cap_v, p["faces"], e.cap_f, p["counts"]), True),
    "mp_mesh_normals": (
        dict(verts="verts", faces="faces", counts="counts"),
        dict(normals=((12 * R * R, 3), F32)),
        lambda e, p: (p["verts"], e.cap_v, p["faces"], e.cap_f, p["counts"], 1, p["normals"]), False),
    "mp_mesh_points": (
        dict(verts="verts", counts="counts"),
        dict(points=((3, 12 * R * R), F32), count_out=((1,), I32)),
        lambda e, p: (p["verts"], e.cap_v, p["counts"], p["points"], p["count_out"]), False),
    "mp_volume_keep_largest": (
        dict(volume="volume"),
        dict(out=((R, R, R), F32), stats=((4,), I32)),
        lambda e, p: (p["volume"], R, 0.5, 6, 0.0, p["out"], p["stats"]), True),
}


def _nbytes(shape, dtype):
    return int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()


def _filled(outs):
    return {k: torch.full((_nbytes(*spec),), FILL, dtype=torch.uint8, device=DEV) for k, spec in outs.items()}


def _call(e, name, tensors, batch):
    ins, outs, args, gated = STAGES[name]
    if batch:
        p = {k: (ctypes.c_void_p * 1)(t.data_ptr()) for k, t in tensors.items()}
        head, tail = (e.h, 1), ((None,) if gated else ())
    else:
        p = {k: ctypes.c_void_p(t.data_ptr()) for k, t in tensors.items()}
        head, tail = (e.h,), ()
    rc = getattr(e.lib, name + ("_batch" if batch else ""))(*head, *args(e, p), *tail, e.st)
    return rc, e.lib.mp_last_error(e.h).decode()


def _untouched(bufs):
    torch.cuda.synchronize()
    return all(bool((b == FILL).all()) for b in bufs.values())


@pytest.mark.parametrize("name", sorted(STAGES))
def test_frame_entry_is_the_batch_entry_with_one_frame(env, name):
    ins, outs, _, _ = STAGES[name]
    inputs = {k: getattr(env, attr) for k, attr in ins.items()}
    got = {}
    for batch in (False, True):
        bufs = _filled(outs)
        rc, msg = _call(env, name, {**inputs, **bufs}, batch)
        assert rc == MP_OK, msg
        torch.cuda.synchronize()
        got[batch] = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k in outs:
        assert np.array_equal(got[False][k], got[True][k]), k
        assert (got[False][k] != FILL).any(), k  # the call wrote something: the comparison is not of two fills
    if name == "mp_volume_keep_largest":
        assert got[False]["stats"].view(np.int32).tolist()[1] == 2  # the ball and the voxel
    # a pointer that is not 4-byte aligned: refused on the host under the entry's own name, whichever argument it is
    bufs = _filled(outs)
    for k, t in {**inputs, **bufs}.items():
        nbytes = t.numel() * t.element_size()
        odd = torch.full((nbytes + 8,), FILL, dtype=torch.uint8, device=DEV)[2:2 + nbytes]
        assert odd.data_ptr() % 4 == 2
        rc, msg = _call(env, name, {**inputs, **bufs, k: odd}, False)
        assert rc == MP_ERR_ARG and msg.startswith(name + ": misaligned buffer for frame 0"), (k, rc, msg)
        assert _untouched(bufs) and bool((odd == FILL).all()), k
    # a null pointer likewise
    for k in {**inputs, **bufs}:
        p = {j: ctypes.c_void_p(t.data_ptr()) for j, t in {**inputs, **bufs}.items()}
        p[k] = None
        rc = getattr(env.lib, name)(env.h, *STAGES[name][2](env, p), env.st)
        msg = env.lib.mp_last_error(env.h).decode()
        assert rc == MP_ERR_ARG and msg.startswith(name + ": null buffer for frame 0"), (k, rc, msg)
    assert _untouched(bufs)


def test_mesh_normals_of_no_vertices_launches_nothing(env):
    bufs = _filled(STAGES["mp_mesh_normals"][1])
    rc = env.lib.mp_mesh_normals(env.h, ctypes.c_void_p(env.verts.data_ptr()), 0, ctypes.c_void_p(env.faces.data_ptr()),
                                 env.cap_f, ctypes.c_void_p(env.counts.data_ptr()), 1,
                                 ctypes.c_void_p(bufs["normals"].data_ptr()), env.st)
    assert rc == MP_OK, env.lib.mp_last_error(env.h).decode()
    assert _untouched(bufs)
    # ... and without rows there is no pointer to look at
    rc = env.lib.mp_mesh_normals(env.h, None, 0, None, 0, ctypes.c_void_p(env.counts.data_ptr()), 1, None, env.st)
    assert rc == MP_OK, env.lib.mp_last_error(env.h).decode()
