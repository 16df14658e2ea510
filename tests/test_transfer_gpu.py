"""mp_volume_bits / mp_mesh_transfer / mp_mesh_transfer_shade (csrc/transfer.hip), mp_picture_light_transfer
(csrc/light.hip), their ops wrappers, recon.mesh_transfer and ``Lighting(transfer=...)`` in the render calls and the
slots, on the GPU.  Every comparison is array_equal on the bits against the numpy restatement (tests/transfer_ref.py,
which visits every sample and knows nothing of blocks), except the gamma step, which is held to the lighting's own
measured tolerance.  No stage here uses the scratch arena, so there is no dirty-arena case.  Needs an MI355X."""
import ctypes
import math

import numpy as np
import pytest

import light_ref
import scene_ref
import transfer_ref as ref
from test_light_gpu import GAMMA_TOL, RASTER, cameras, mesh_counts, params, synthetic
from test_mesh_batch_gpu import nets  # noqa: F401  (the fixture)
from test_mesh_render_gpu import ARG, DEV, OK, UNSUPPORTED, bits, host
from test_render_netc_gpu import PICTURES as NETC_PICTURES, colour_slot, own_maps, slot_cameras  # noqa: F401
from test_render_netc_gpu import views_frames, views_net, views_netc  # noqa: F401  (the fixtures of the multi-view nets)
from test_scene_gpu import procedural

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
BG = 0.25
PICTURES = [(33, 20), (20, 48)]
PF = ctypes.POINTER(ctypes.c_float)
UNIT = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
SKEW = ((-1.0, -1.5, -0.8), (1.2, 1.5, 1.0))  # three different edges: 2.2, 3.0, 1.8


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)  # a copy: the cases' arrays are read-only


def same(got, want):
    got = host(got) if torch.is_tensor(got) else got
    want = host(want) if torch.is_tensor(want) else want
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return np.array_equal(bits(got), bits(want)) if got.dtype == F else np.array_equal(got, want)


def u64(t):
    return host(t).view(np.uint64)


# ---- the cases: computed once, shared, never changed ------------------------------------------------------------------
def surface(vol, box):
    """The oracle's marching cubes of a volume with the accumulated normals, and five rows that no mesh has: a zero, a
    NaN and an inf normal, a vertex outside the box and a NaN vertex."""
    from monoport_amd import mesh_util
    from oracle import pifu_oracle
    v, f = pifu_oracle.marching_cubes(vol, 0.5, *box)
    v = np.ascontiguousarray(v, F)
    n = np.ascontiguousarray(mesh_util.compute_normal(v, np.ascontiguousarray(f, np.int32), "accumulate"), F)
    return odd_rows(v, n, box)


def odd_rows(v, n, box):
    lo, hi = np.asarray(box[0], F), np.asarray(box[1], F)
    mid = (lo + hi) / 2
    v = np.concatenate([v, [mid, mid, mid, hi + (hi - lo) * F(0.25), [np.nan, mid[1], mid[2]]]]).astype(F)
    n = np.concatenate([n, [[0, 0, 0], [np.nan, 1, 0], [0, np.inf, 0], [0, 0, -1], [0, 0, 1]]]).astype(F)
    if v.shape[0] % 64 == 0:  # a count that is no multiple of the wavefront
        v, n = v[1:], n[1:]
    return v, n


def scattered(r, box, count=333, seed=0):
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(box[0], F), np.asarray(box[1], F)
    return odd_rows((lo + (hi - lo) * rng.uniform(0, 1, (count, 3))).astype(F),
                    rng.standard_normal((count, 3)).astype(F), box)


CASES = {
    # name: (volume, box, D, bias, step, reach)
    "blob17": (lambda: ref.sphere_with_blob(17), UNIT, 64, 1.5, 1.0, None),
    "blob33_skew_box": (lambda: ref.sphere_with_blob(33), SKEW, 128, 1.5, 1.0, None),
    "corner33_bias0_step_half": (lambda: ref.corner(33), UNIT, 64, 0.0, 0.5, None),
    "blob33_short_reach": (lambda: ref.sphere_with_blob(33), UNIT, 64, 1.5, 1.0, 6.0),
    "empty17": (lambda: np.zeros((17, 17, 17), F), UNIT, 64, 1.5, 1.0, None),
    "full17": (lambda: np.ones((17, 17, 17), F), SKEW, 128, 1.5, 1.0, None),
}


class Case:
    def __init__(self, name):
        make, self.box, self.d, bias, step, reach = CASES[name]
        self.vol = make()
        self.r = self.vol.shape[0]
        self.verts, self.normals = (scattered(self.r, self.box) if name in ("empty17", "full17")
                                    else surface(self.vol, self.box))
        self.dirs, self.basis, self.weight = ref.tables(self.d)
        self.bias_w, self.step_w, self.steps = ref.rays(self.r, *self.box, bias=bias, step=step, reach=reach)
        self.mask, self.prt, self.samples = ref.transfer(self.verts, self.normals, ref.occupancy(self.vol, 0.5),
                                                         *self.box, self.dirs, self.basis, self.weight, self.bias_w,
                                                         self.step_w, self.steps)
        for a in (self.vol, self.verts, self.normals, self.mask, self.prt):
            a.setflags(write=False)

    def args(self):
        return (self.r, self.box[0], self.box[1], dev(self.dirs), dev(self.basis), float(self.weight),
                float(self.bias_w), float(self.step_w), self.steps)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name)
        return made[name]
    return get


def counts_of(nv, nf=0):
    return torch.tensor([nv, nf], dtype=torch.int32, device=DEV)


# ---- the bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 17, 33, 65])
def test_bits_against_the_restatement(ops, r):
    """Random volumes with NaN, inf and == level voxels; 33 has a one-voxel last block, 65 an odd number of words per
    row.  The buffer is a slice between two guards."""
    rng = np.random.RandomState(r)
    vol = rng.uniform(0, 1, (r, r, r)).astype(F)
    flat = vol.reshape(-1)
    flat[rng.randint(0, flat.size, max(1, flat.size // 7))] = np.nan
    flat[rng.randint(0, flat.size, max(1, flat.size // 9))] = F(0.5)
    flat[-1] = np.inf
    fine, words = ref.bits_words(r)
    assert ops.volume_bits_words(r) == words
    guard = torch.full((words + 128,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    got = ops.volume_bits_raw(dev(vol), 0.5, out=guard[64:64 + words])
    assert got.data_ptr() == guard[64:].data_ptr()
    want = ref.volume_bits(vol, 0.5)
    assert np.array_equal(host(got)[:fine].view(np.uint32), want)
    assert (guard[:64] == 0x5A5A5A5A).all() and (guard[64 + words:] == 0x5A5A5A5A).all()
    fresh = ops.volume_bits_raw(dev(vol), 0.5)
    assert torch.equal(fresh, got)  # the private words too: a pure function of the volume
    # another level is other bits
    assert np.array_equal(host(ops.volume_bits_raw(dev(vol), 0.25))[:fine].view(np.uint32), ref.volume_bits(vol, 0.25))


def test_bits_batched_and_gated(ops):
    vols = [ref.sphere_with_blob(33), np.zeros((33, 33, 33), F), np.ones((33, 33, 33), F), ref.corner(33)]
    fine, words = ref.bits_words(33)
    singles = [ops.volume_bits_raw(dev(v), 0.5) for v in vols]
    batch = ops.volume_bits_raw_batch([dev(v) for v in vols], 0.5)
    assert all(torch.equal(a, b) for a, b in zip(batch, singles))
    assert not host(singles[1]).any() and (host(singles[2])[:fine:2] == -1).all()
    on, off = counts_of(1)[:1], counts_of(0)[:1]
    out = torch.full((4, words), 7, dtype=torch.int32, device=DEV)
    poisoned = torch.full((33, 33, 33), float("nan"), device=DEV)  # a gated-off frame is not read either
    got = ops.volume_bits_raw_batch([dev(vols[0]), poisoned, dev(vols[2]), dev(vols[3])], 0.5,
                                    gates=[on, off, None, off], out=out)
    assert torch.equal(got[0], singles[0]) and torch.equal(got[2], singles[2])
    assert (out[1] == 7).all() and (out[3] == 7).all()


# ---- the transfer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_transfer_against_the_restatement(ops, cases, name):
    c = cases(name)
    nv = c.verts.shape[0]
    assert nv % 64 != 0 and nv > 64
    bits_ = ops.volume_bits_raw(dev(c.vol), 0.5)
    cap = nv + 70  # rows beyond the count keep what they held
    verts = torch.zeros((cap, 3), device=DEV)
    normals = torch.zeros((cap, 3), device=DEV)
    verts[:nv], normals[:nv] = dev(c.verts), dev(c.normals)
    normals[nv:] = 1.0
    mask = torch.full((cap, c.d // 64), -7, dtype=torch.int64, device=DEV)
    prt = torch.full((cap, 9), -7.0, device=DEV)
    got = ops.mesh_transfer_raw(verts, normals, counts_of(nv), bits_, *c.args(), out=(mask, prt))
    assert got[0].data_ptr() == mask.data_ptr() and got[1].data_ptr() == prt.data_ptr()
    assert np.array_equal(u64(mask[:nv]), c.mask)
    assert same(prt[:nv], c.prt)
    assert (mask[nv:] == -7).all() and (prt[nv:] == -7.0).all()
    # what the case is there for
    seen = np.unpackbits(c.mask.view(np.uint8), bitorder="little").reshape(nv, -1).astype(bool)
    with np.errstate(invalid="ignore"):
        facing = (light_ref.normalise(c.normals) @ c.dirs.T) > 0
    if name == "empty17":
        assert np.array_equal(seen, facing)
    elif name == "full17":  # only a ray whose biased origin lies outside the box gets away
        assert (facing & ~seen).sum() > (facing & seen).sum() and not (seen & ~facing).any()
    else:
        assert (facing & ~seen).any() and (facing & seen).any() and not (seen & ~facing).any()
    assert not c.prt[nv - 5:nv - 2].any() and not seen[nv - 5:nv - 2].any()  # zero, NaN and inf normals
    assert np.array_equal(seen[nv - 2:], facing[nv - 2:])  # outside the box, a NaN position: left at once
    # one output alone, fresh buffers
    only_mask = ops.mesh_transfer_raw(verts, normals, counts_of(nv), bits_, *c.args(), want=(True, False))
    only_prt = ops.mesh_transfer_raw(verts, normals, counts_of(nv), bits_, *c.args(), want=(False, True))
    assert only_mask[1] is None and only_prt[0] is None
    assert np.array_equal(u64(only_mask[0][:nv]), c.mask) and same(only_prt[1][:nv], c.prt)


def test_transfer_skips_exactly_what_is_empty(ops, cases):
    """A reach of J = 1 .. a few samples on the blob: each J is its own truth (a skip that overshoots the reach, or a
    block test off by one, shows as a bit), and a count of 0 writes nothing."""
    c = cases("blob33_short_reach")
    nv = c.verts.shape[0]
    occ = ref.occupancy(c.vol, 0.5)
    bits_ = ops.volume_bits_raw(dev(c.vol), 0.5)
    verts, normals = dev(c.verts), dev(c.normals)
    args = list(c.args())
    for steps in (1, 2, 9, 17):
        args[-1] = steps
        want = ref.transfer(c.verts, c.normals, occ, *c.box, c.dirs, c.basis, c.weight, c.bias_w, c.step_w, steps)
        got = ops.mesh_transfer_raw(verts, normals, counts_of(nv), bits_, *args)
        assert np.array_equal(u64(got[0]), want[0]) and same(got[1], want[1]), steps
    mask = torch.full((nv, 1), -7, dtype=torch.int64, device=DEV)
    prt = torch.full((nv, 9), -7.0, device=DEV)
    for count in (0, -3):
        ops.mesh_transfer_raw(verts, normals, counts_of(count), bits_, *c.args(), out=(mask, prt))
    assert (mask == -7).all() and (prt == -7.0).all()
    # a count beyond the capacity serves the capacity
    got = ops.mesh_transfer_raw(verts, normals, counts_of(nv + 1000), bits_, *c.args())
    assert np.array_equal(u64(got[0]), c.mask) and same(got[1], c.prt)


def test_transfer_batched_equals_per_frame(ops, cases):
    a, b = cases("blob33_short_reach"), cases("corner33_bias0_step_half")
    nv = min(a.verts.shape[0], b.verts.shape[0])
    args = a.args()
    vols = [a.vol, b.vol, np.zeros((33, 33, 33), F), a.vol]
    frames = [(a.verts[:nv], a.normals[:nv], nv), (b.verts[:nv], b.normals[:nv], nv - 37), (a.verts[:nv], a.normals[:nv], 0),
              (b.verts[:nv], b.normals[:nv], 100)]
    bits_ = ops.volume_bits_raw_batch([dev(v) for v in vols], 0.5)
    verts, normals = [dev(f[0]) for f in frames], [dev(f[1]) for f in frames]
    counts = [counts_of(f[2]) for f in frames]
    mask = torch.full((4, nv, 1), -7, dtype=torch.int64, device=DEV)
    prt = torch.full((4, nv, 9), -7.0, device=DEV)
    got = ops.mesh_transfer_raw_batch(verts, normals, counts, bits_, *args, out=(mask, prt))
    for f, (v, n, count) in enumerate(frames):
        single = ops.mesh_transfer_raw(verts[f], normals[f], counts[f], bits_[f], *args)
        assert torch.equal(got[f][0][:count], single[0][:count]) and same(got[f][1][:count], single[1][:count])
        assert (mask[f, count:] == -7).all() and (prt[f, count:] == -7.0).all()
        want = ref.transfer(v[:count], n[:count], ref.occupancy(vols[f], 0.5), *a.box, a.dirs, a.basis, a.weight, a.bias_w,
                            a.step_w, a.steps)
        assert np.array_equal(u64(mask[f, :count]), want[0]) and same(prt[f, :count], want[1])


def test_shade_against_the_restatement(ops, cases):
    c = cases("blob33_skew_box")
    nv = c.verts.shape[0]
    sh = params(4)[0]
    prt = torch.full((nv + 9, 9), float("nan"), device=DEV)
    prt[:nv] = dev(c.prt)
    out = torch.full((nv + 9, 3), -7.0, device=DEV)
    got = ops.mesh_transfer_shade_raw(prt, counts_of(nv), sh, out=out)
    assert got.data_ptr() == out.data_ptr() and same(out[:nv], ref.shade(c.prt, sh)) and (out[nv:] == -7.0).all()
    # batched, with an empty frame
    outs = ops.mesh_transfer_shade_raw_batch([prt, prt, prt], [counts_of(nv), counts_of(0), counts_of(65)], sh,
                                             out=torch.full((3, nv + 9, 3), -7.0, device=DEV))
    assert same(outs[0][:nv], ref.shade(c.prt, sh)) and (outs[1] == -7.0).all()
    assert same(outs[2][:65], ref.shade(c.prt[:65], sh)) and (outs[2][65:] == -7.0).all()


# ---- the lighting entry point -----------------------------------------------------------------------------------------
def ambient_of(size, seed=0):
    rng = np.random.RandomState(100 + seed)
    amb = rng.uniform(-0.3, 1.6, (2,) + tuple(size) + (3,)).astype(F)
    amb.reshape(-1, 3)[3] = [np.nan, -0.0, np.inf]
    return amb


@pytest.mark.parametrize("size", PICTURES, ids=lambda s: "%dx%d" % s)
def test_light_transfer_against_the_restatement(ops, size):
    normal, face, albedo, vis = synthetic(size)
    amb = ambient_of(size)
    _, direct, _ = params()
    d = [dev(a) for a in (amb, normal, face, albedo, vis)]
    for with_direct in (False, True):
        for with_vis in (False, True):
            kw = dict(direct=direct if with_direct else None, visibilities=[d[4]] if with_vis else None)
            rkw = dict(direct_dir=direct[0] if with_direct else None, direct_rgb=direct[1] if with_direct else None,
                       visibility=vis if with_vis else None)
            image, shading = ops.picture_light_transfer_batch([d[0]], [d[1]], [d[2]], [d[3]], with_shading=True, **kw)[0]
            want = ref.light_transfer(amb, normal, face, albedo, **rkw)
            assert same(image, want[0].reshape(image.shape)) and same(shading, want[1].reshape(shading.shape))
            if not with_direct:  # the normals are not read
                none = ops.picture_light_transfer_batch([d[0]], None, [d[2]], [d[3]], with_shading=True, **kw)[0]
                assert same(none[0], image) and same(none[1], shading)
    # a constant albedo, the background, in place
    image, _ = ops.picture_light_transfer_batch([d[0]], [d[1]], [d[2]], None, direct=direct, albedo_rgb=(0.8, 0.7, 0.6),
                                                background=BG)[0]
    want = ref.light_transfer(amb, normal, face, None, direct[0], direct[1], albedo_rgb=(0.8, 0.7, 0.6), background=BG)
    assert same(image, want[0].reshape(image.shape))
    place = d[3].clone()
    ops.picture_light_transfer_batch([d[0]], [d[1]], [d[2]], [place], direct=direct, out=([place], None))
    assert same(place, ref.light_transfer(amb, normal, face, albedo, direct[0], direct[1])[0].reshape(place.shape))
    # batched == per frame
    amb2 = dev(ambient_of(size, 1))
    both = ops.picture_light_transfer_batch([d[0], amb2], [d[1], d[1]], [d[2], d[2]], [d[3], d[3]], direct=direct)
    one = ops.picture_light_transfer_batch([amb2], [d[1]], [d[2]], [d[3]], direct=direct)
    assert same(both[1][0], one[0][0])
    # mp_picture_light itself keeps its bits beside the new form
    sh = params()[0]
    lit = ops.picture_light_batch([d[1]], [d[2]], [d[3]], sh, direct=direct)[0][0]
    assert same(lit, light_ref.light(normal, face, albedo, sh, direct[0], direct[1], n_views=2)[0].reshape(lit.shape))


@pytest.mark.parametrize("size", PICTURES, ids=lambda s: "%dx%d" % s)
def test_light_transfer_gamma_against_float64(ops, size):
    normal, face, albedo, vis = synthetic(size)
    amb = ambient_of(size)
    _, direct, _ = params()
    image, shading = ops.picture_light_transfer_batch([dev(amb)], [dev(normal)], [dev(face)], [dev(albedo)], direct=direct,
                                                      gamma=2.2, visibilities=[dev(vis)], with_shading=True)[0]
    want = ref.light_transfer(amb, normal, face, albedo, direct[0], direct[1], gamma=2.2, visibility=vis, dtype=np.float64)
    ok = np.isfinite(want[1]).all(1) & np.isfinite(want[0]).all(1)
    e_shading = np.abs(host(shading).reshape(-1, 3)[ok] - want[1][ok]).max()
    e_image = np.abs(host(image).reshape(-1, 3)[ok] - want[0][ok]).max()
    print("gamma 2.2 at %s: shading %.3g image %.3g" % (size, e_shading, e_image))
    assert ok.sum() > 100 and e_shading <= GAMMA_TOL and e_image <= GAMMA_TOL


# ---- refusals through the C ABI ---------------------------------------------------------------------------------------
class Env:
    """Well-formed calls of the four entry points on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
        self.r = 9
        self.words = ops.volume_bits_words(9)
        self.vol, self.bits = z(9, 9, 9), z(self.words + 2, dtype=torch.int32)
        self.verts, self.normals, self.counts = z(70, 3), z(70, 3), torch.tensor([70, 0], dtype=torch.int32, device=DEV)
        self.normals[:, 2] = 1.0
        self.mask, self.prt, self.shade = z(70, 1, dtype=torch.int64), z(70, 9), z(70, 3)
        dirs, basis, _ = ref.tables(64)
        self.dirs, self.basis = dev(dirs), dev(basis)
        self.lo, self.hi, self.sh = np.array([-1, -1, -1], F), np.array([1, 1, 1], F), np.ones((9, 3), F)
        self.n = 24
        self.amb, self.pnormal, self.albedo, self.out, self.shading = (z(24, 3) for _ in range(5))
        self.vis, self.face = z(24), z(24, dtype=torch.int32)
        self.dir, self.rgb, self.const = np.array([0, 0, -1], F), np.full(3, 0.5, F), np.ones(3, F)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def done(self, rc):
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()

    @staticmethod
    def pf(a):
        return PF() if a is None else a.ctypes.data_as(PF)

    def volume_bits(self, **k):
        a = dict(vol=self.vol.data_ptr(), r=self.r, bits=self.bits.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_volume_bits(self.ctx.handle, a["vol"], a["r"], 0.5, a["bits"], self.stream))

    def transfer(self, **k):
        a = dict(verts=self.verts.data_ptr(), normals=self.normals.data_ptr(), max_v=70, counts=self.counts.data_ptr(),
                 bits=self.bits.data_ptr(), r=self.r, lo=self.lo, hi=self.hi, d=64, dirs=self.dirs.data_ptr(),
                 basis=self.basis.data_ptr(), weight=0.2, bias=0.3, step=0.2, steps=20, mask=self.mask.data_ptr(),
                 prt=self.prt.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_mesh_transfer(
            self.ctx.handle, a["verts"], a["normals"], a["max_v"], a["counts"], a["bits"], a["r"], self.pf(a["lo"]),
            self.pf(a["hi"]), a["d"], a["dirs"], a["basis"], a["weight"], a["bias"], a["step"], a["steps"], a["mask"],
            a["prt"], self.stream))

    def shade_(self, **k):
        a = dict(prt=self.prt.data_ptr(), max_v=70, counts=self.counts.data_ptr(), sh=self.sh, out=self.shade.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_mesh_transfer_shade(self.ctx.handle, a["prt"], a["max_v"], a["counts"],
                                                         self.pf(a["sh"]), a["out"], self.stream))

    def light(self, **k):
        a = dict(normal=self.pnormal.data_ptr(), face=self.face.data_ptr(), albedo=self.albedo.data_ptr(), const=None,
                 vis=self.vis.data_ptr(), amb=self.amb.data_ptr(), n=self.n, dir=self.dir, rgb=self.rgb, gamma=1.0,
                 background=1.0, out=self.out.data_ptr(), shading=self.shading.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_light_transfer(
            self.ctx.handle, a["normal"], a["face"], a["albedo"], self.pf(a["const"]), a["vis"], a["amb"], a["n"],
            self.pf(a["dir"]), self.pf(a["rgb"]), a["gamma"], a["background"], a["out"], a["shading"], self.stream))


def check_refusals(call, name, refused):
    for changed, code, word in refused:
        rc, msg = call(**changed)
        assert rc == code and msg.startswith(name + ":") and word in msg, (changed, rc, msg)


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    lib, h = env.lib, env.ctx.handle
    assert lib.mp_volume_bits_words(9) == env.words and lib.mp_volume_bits_words(513) == ref.bits_words(513)[1]
    assert lib.mp_volume_bits_words(0) == 0 and lib.mp_volume_bits_words(514) == 0
    assert env.volume_bits()[0] == OK and env.transfer()[0] == OK and env.shade_()[0] == OK and env.light()[0] == OK
    assert env.transfer(mask=None)[0] == OK and env.transfer(prt=None)[0] == OK and env.transfer(max_v=0)[0] == OK
    assert env.light(normal=None, rgb=np.zeros(3, F))[0] == OK and env.shade_(max_v=0)[0] == OK
    torch.cuda.synchronize()
    outs = (env.bits, env.mask, env.prt, env.shade, env.out, env.shading)
    for t in outs:
        t.fill_(5)
    nan = lambda a, i: np.where(np.arange(a.size).reshape(a.shape) == i, F(np.nan), a).astype(F)  # noqa: E731
    check_refusals(env.volume_bits, "mp_volume_bits", [
        (dict(r=0), ARG, "resolution"), (dict(r=514), ARG, "resolution"), (dict(vol=None), ARG, "null"),
        (dict(bits=None), ARG, "null"), (dict(bits=env.bits.data_ptr() + 2), ARG, "misaligned"),
        (dict(vol=env.vol.data_ptr() + 1), ARG, "misaligned"), (dict(bits=env.vol.data_ptr() + 8), ARG, "aliases"),
    ])
    check_refusals(env.transfer, "mp_mesh_transfer", [
        (dict(r=0), ARG, "resolution"), (dict(r=514), ARG, "resolution"),
        (dict(d=0), ARG, "n_dirs"), (dict(d=96), ARG, "n_dirs"), (dict(d=576), ARG, "n_dirs"),
        (dict(steps=0), ARG, "max_steps"), (dict(steps=(1 << 24) + 1), ARG, "max_steps"),
        (dict(lo=None), ARG, "bad argument"), (dict(hi=None), ARG, "bad argument"), (dict(dirs=None), ARG, "bad argument"),
        (dict(basis=None), ARG, "bad argument"), (dict(max_v=-1), ARG, "bad argument"),
        (dict(verts=None), ARG, "null"), (dict(normals=None), ARG, "null"), (dict(counts=None), ARG, "null"),
        (dict(bits=None), ARG, "null"),
        (dict(lo=nan(env.lo, 1)), ARG, "b_min"), (dict(hi=np.array([1, -1, 1], F)), ARG, "b_min"),
        (dict(hi=np.array([1, np.inf, 1], F)), ARG, "b_min"),
        (dict(weight=math.nan), ARG, "step_w"), (dict(bias=math.inf), ARG, "step_w"), (dict(step=0.0), ARG, "step_w"),
        (dict(step=-0.2), ARG, "step_w"), (dict(step=math.nan), ARG, "step_w"),
        (dict(mask=None, prt=None), ARG, "no output"),
        (dict(max_v=0x7fffffff // 9 + 1), UNSUPPORTED, "2^31 / 9"),
        (dict(dirs=env.dirs.data_ptr() + 2), ARG, "misaligned"), (dict(verts=env.verts.data_ptr() + 1), ARG, "misaligned"),
        (dict(mask=env.mask.data_ptr() + 4), ARG, "mask"), (dict(prt=env.prt.data_ptr() + 2), ARG, "misaligned"),
        (dict(prt=env.verts.data_ptr()), ARG, "aliases"), (dict(mask=env.normals.data_ptr()), ARG, "aliases"),
        (dict(prt=env.bits.data_ptr()), ARG, "aliases"), (dict(mask=env.prt.data_ptr()), ARG, "aliases"),
        (dict(mask=env.counts.data_ptr()), ARG, "aliases"),
        (dict(prt=env.dirs.data_ptr()), ARG, "dirs or basis"), (dict(mask=env.basis.data_ptr() + 8), ARG, "dirs or basis"),
        (dict(prt=env.basis.data_ptr() + 64 * 36 - 4), ARG, "dirs or basis"),
    ])
    check_refusals(env.shade_, "mp_mesh_transfer_shade", [
        (dict(sh=None), ARG, "bad argument"), (dict(max_v=-1), ARG, "bad argument"), (dict(counts=None), ARG, "null"),
        (dict(prt=None), ARG, "null"), (dict(out=None), ARG, "null"), (dict(sh=nan(env.sh, 13)), ARG, "finite"),
        (dict(max_v=0x7fffffff // 9 + 1), UNSUPPORTED, "2^31 / 9"), (dict(out=env.shade.data_ptr() + 2), ARG, "misaligned"),
        (dict(out=env.prt.data_ptr()), ARG, "aliases"),
    ])
    check_refusals(env.light, "mp_picture_light_transfer", [
        (dict(n=0), ARG, "n_pixels"), (dict(n=0x7fffffff // 3 + 1), UNSUPPORTED, "2^31 / 3"),
        (dict(amb=None), ARG, "bad argument"), (dict(dir=None), ARG, "bad argument"), (dict(rgb=None), ARG, "bad argument"),
        (dict(const=env.const), ARG, "both"), (dict(albedo=None), ARG, "neither"),
        (dict(gamma=0.0), ARG, "gamma"), (dict(gamma=math.nan), ARG, "gamma"),
        (dict(dir=nan(env.dir, 1)), ARG, "finite"), (dict(rgb=np.array([0, np.inf, 0], F)), ARG, "finite"),
        (dict(background=math.nan), ARG, "finite"), (dict(out=None, shading=None), ARG, "no output"),
        (dict(normal=None), ARG, "direct term"), (dict(face=None), ARG, "null"),
        (dict(amb=env.amb.data_ptr() + 2), ARG, "misaligned"),
        (dict(out=env.amb.data_ptr()), ARG, "aliases"), (dict(shading=env.amb.data_ptr() + 12), ARG, "aliases"),
        (dict(out=env.pnormal.data_ptr()), ARG, "aliases"), (dict(shading=env.out.data_ptr()), ARG, "aliases"),
        (dict(out=env.albedo.data_ptr() + 12), ARG, "aliases"),
    ])
    torch.cuda.synchronize()
    assert all((t == 5).all() for t in outs)  # nothing was launched
    assert env.light(out=env.albedo.data_ptr(), shading=None)[0] == OK  # in place stays allowed
    # the batched forms carry their own names and refuse a frame count out of range; two frames may share no output
    ptr = (ctypes.c_void_p * 2)(env.prt.data_ptr(), env.prt.data_ptr())
    for n_frames in (0, 33):
        for call, name in (
                (lambda n: lib.mp_volume_bits_batch(h, n, ptr, 9, 0.5, ptr, None, env.stream), "mp_volume_bits_batch"),
                (lambda n: lib.mp_mesh_transfer_batch(h, n, ptr, ptr, 70, ptr, ptr, 9, env.pf(env.lo), env.pf(env.hi), 64,
                                                      env.dirs.data_ptr(), env.basis.data_ptr(), 0.2, 0.3, 0.2, 20, ptr,
                                                      ptr, env.stream), "mp_mesh_transfer_batch"),
                (lambda n: lib.mp_mesh_transfer_shade_batch(h, n, ptr, 70, ptr, env.pf(env.sh), ptr, env.stream),
                 "mp_mesh_transfer_shade_batch"),
                (lambda n: lib.mp_picture_light_transfer_batch(h, n, ptr, ptr, ptr, PF(), ptr, ptr, 24, env.pf(env.dir),
                                                               env.pf(env.rgb), 1.0, 1.0, ptr, ptr, env.stream),
                 "mp_picture_light_transfer_batch")):
            rc, msg = env.done(call(n_frames))
            assert rc == ARG and msg.startswith(name + ":"), (name, rc, msg)
    arr = lambda *ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])  # noqa: E731
    rc = lib.mp_volume_bits_batch(h, 2, arr(env.vol, env.vol), 9, 0.5, arr(env.bits, env.bits), None, env.stream)
    assert env.done(rc)[0] == ARG and "aliases an output" in env.done(rc)[1]
    rc = lib.mp_mesh_transfer_shade_batch(h, 2, arr(env.prt, env.prt), 70, arr(env.counts, env.counts), env.pf(env.sh),
                                          arr(env.shade, env.shade), env.stream)
    assert env.done(rc)[0] == ARG and "aliases an output" in env.done(rc)[1]
    rc = lib.mp_mesh_transfer_batch(h, 2, arr(env.verts, env.verts), arr(env.normals, env.normals), 70,
                                    arr(env.counts, env.counts), arr(env.bits, env.bits), 9, env.pf(env.lo),
                                    env.pf(env.hi), 64, env.dirs.data_ptr(), env.basis.data_ptr(), 0.2, 0.3, 0.2, 20,
                                    arr(env.mask, env.mask), None, env.stream)
    assert env.done(rc)[0] == ARG and "aliases an output" in env.done(rc)[1]


def test_ops_refuses_before_it_enqueues(ops, cases):
    c = cases("blob17")
    nv = c.verts.shape[0]
    verts, normals, bits_ = dev(c.verts), dev(c.normals), ops.volume_bits_raw(dev(c.vol), 0.5)
    args = list(c.args())

    def call(i=None, value=None, **k):
        a = list(args)
        if i is not None:
            a[i] = value
        return ops.mesh_transfer_raw(k.pop("verts", verts), k.pop("normals", normals), k.pop("counts", counts_of(nv)),
                                     k.pop("bits", bits_), *a, **k)
    for kw in (dict(i=0, value=33), dict(i=0, value=0), dict(i=1, value=(1, 1, 1)), dict(i=3, value=dev(c.dirs)[:32]),
               dict(i=4, value=dev(c.basis)[:, :3]), dict(i=3, value=c.dirs), dict(i=5, value=math.nan),
               dict(i=7, value=0.0), dict(i=8, value=0), dict(want=(False, False)), dict(normals=normals[:-1]),
               dict(bits=bits_[:-1]), dict(bits=bits_.float()), dict(counts=counts_of(nv).long()),
               dict(out=(torch.zeros((nv, 1), dtype=torch.int32, device=DEV), None)),
               dict(out=(None, torch.zeros((nv, 3), device=DEV)))):
        with pytest.raises((ValueError, RuntimeError)):
            call(**kw)
    with pytest.raises(ValueError):
        ops.volume_bits_raw(torch.zeros((4, 4, 5), device=DEV))
    with pytest.raises(ValueError):
        ops.volume_bits_raw(torch.zeros((4, 4, 4), device=DEV), out=torch.zeros(3, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.mesh_transfer_shade_raw(dev(c.prt), counts_of(nv), np.zeros((3, 9), F))
    amb = torch.zeros((4, 4, 3), device=DEV)
    face = torch.zeros((4, 4), dtype=torch.int32, device=DEV)
    for kw in (dict(direct=((0, 0, -1), (1, 1, 1))), dict(albedo_rgb=None), dict(gamma=0.0), dict(background=math.inf),
               dict(out=(None, None))):
        with pytest.raises((ValueError, RuntimeError)):
            ops.picture_light_transfer_batch([amb], None, [face], None, **dict(dict(albedo_rgb=(1, 1, 1)), **kw))


# ---- the whole path: recon.mesh_transfer and the render calls ---------------------------------------------------------
@pytest.fixture(scope="module")
def world(recon):
    """The blob over the ball at 33^3 as a Mesh with its transfer, a second mesh (the corner) and a scene."""
    import shadow_cases
    from oracle import pifu_oracle
    from monoport_amd import mesh_util
    made = {}
    for name, vol in (("blob", ref.sphere_with_blob(33)), ("corner", ref.corner(33))):
        v, f = pifu_oracle.marching_cubes(vol)
        v, f = np.ascontiguousarray(v, F), np.ascontiguousarray(f, np.int32)
        n = np.ascontiguousarray(mesh_util.compute_normal(v, f, "accumulate"), F)
        made[name] = (vol, recon.Mesh(dev(v), dev(f), dev(n), dev((v * F(0.4) + F(0.5)).astype(F))))
    fv, ff, uv = shadow_cases.plank(x=(-2.0, 3.0), z=(-1.5, 1.5))
    made["scene"] = recon.Scene(fv, ff, uv, procedural(64, 64), device=DEV)
    return made


def want_transfer(mesh, vol, t):
    bias_w, step_w, steps = ref.rays(vol.shape[0], *UNIT, bias=t.bias, step=t.step, reach=t.reach)
    return ref.transfer(host(mesh.verts), host(mesh.normals), ref.occupancy(vol, 0.5), *UNIT, t.dirs, t.basis,
                        F(t.weight), bias_w, step_w, steps)


def test_recon_mesh_transfer(recon, world):
    t = recon.Transfer(64, bias=1.5, step=1.0)
    vol, mesh = world["blob"]
    prt, mask = recon.mesh_transfer(mesh, dev(vol), t)
    want = want_transfer(mesh, vol, t)
    assert prt.shape == (mesh.verts.shape[0], 9) and mask.shape == (mesh.verts.shape[0], 1) and mask.dtype == torch.int64
    assert np.array_equal(u64(mask), want[0]) and same(prt, want[1])
    # the engines' [1,1,R,R,R] volumes, another level, a reach
    short = recon.Transfer(64, reach=5)
    prt5, _ = recon.mesh_transfer(mesh, dev(vol)[None, None], short, level=0.5)
    assert same(prt5, want_transfer(mesh, vol, short)[1]) and not same(prt5, prt)
    assert np.array_equal(host(recon.volume_bits(dev(vol)))[:ref.bits_words(33)[0]].view(np.uint32),
                          ref.volume_bits(vol, 0.5))
    # the blob's shade: under it the ball sees less sky than on its flanks
    v = host(mesh.verts)
    top_of_ball = (np.abs(v[:, 0] - 0.1) < 0.1) & (np.abs(v[:, 1] + 0.05) < 0.1) & (v[:, 2] > 0.2) & (v[:, 2] < 0.4)
    flank = (np.abs(v[:, 2] + 0.2) < 0.1) & (np.linalg.norm(v[:, :2], axis=1) > 0.45)
    assert top_of_ball.sum() > 3 and flank.sum() > 10
    # right under the blob (radius 0.22, its centre 0.33 above the ball's top) it hides sin^2(42 deg) = 45 % of the
    # cosine-weighted sky; at the window's edge less
    assert host(prt)[top_of_ball, 0].max() < host(prt)[flank, 0].min()
    assert host(prt)[top_of_ball, 0].min() < 0.5 * host(prt)[flank, 0].min()
    empty = recon.Mesh(mesh.verts[:0], mesh.faces[:0], mesh.normals[:0], None)
    assert recon.mesh_transfer(empty, dev(vol), t)[0].shape == (0, 9)


@pytest.mark.parametrize("shade", ["colors", "normals"])
def test_lit_pictures_with_transfer_against_the_restatements(ops, recon, world, shade):
    t = recon.Transfer(64)
    sh, direct, _ = params(3)
    lighting = recon.Lighting(sh, direct=direct, transfer=t, albedo=(0.8, 0.7, 0.6) if shade == "normals" else None)
    plain = recon.Lighting(sh, direct=direct, albedo=lighting.albedo)
    cams, size = cameras(), (66, 40)  # the near plane cuts both bodies: at 33 x 20 one of them covers 30 pixels only
    kw = dict(background=BG, **RASTER)
    meshes = [recon.with_transfer(m, recon.mesh_transfer(m, dev(vol), t)[0]) for vol, m in (world["blob"], world["corner"])]
    got = recon.render_mesh_many([meshes[0], None, meshes[1]], cams, size, shade, lighting=lighting, **kw)
    assert got[1] is None
    for mesh, (vol, bare), picture in zip(meshes, (world["blob"], world["corner"]), (got[0], got[2])):
        front = recon.render_mesh(bare, cams, size, shade, **kw)
        counts = mesh_counts(mesh)
        tvals = ref.shade(want_transfer(bare, vol, t)[1], sh)
        assert same(ops.mesh_transfer_shade_raw(mesh.transfer, counts, sh), tvals)
        nrm = ops.mesh_render_raw(mesh.verts, mesh.faces, counts, mesh.normals, cams, size, background=BG, **RASTER)
        amb = ops.mesh_render_raw(mesh.verts, mesh.faces, counts, dev(tvals), cams, size, background=BG, **RASTER)
        assert torch.equal(amb[2], front.face) and (front.face >= 0).sum() > 100
        want_image, _ = ref.light_transfer(host(amb[0]), host(nrm[0]), host(nrm[2]),
                                           None if shade == "normals" else host(front.image), lighting.direct_dir,
                                           lighting.direct_rgb, albedo_rgb=lighting.albedo, background=BG)
        assert same(picture.image, want_image.reshape(2, *size, 3))
        assert torch.equal(picture.face, front.face) and same(picture.depth, front.depth)
        unoccluded = recon.render_mesh(bare, cams, size, shade, lighting=plain, **kw)
        assert not same(picture.image, unoccluded.image)
    single = recon.render_mesh(meshes[0], cams[1], size, shade, lighting=lighting, **kw)
    assert same(single.image, got[0].image[1])
    # without transfer the parent's call is untouched by a mesh that carries one
    assert same(recon.render_mesh(meshes[0], cams, size, shade, lighting=plain, **kw).image,
                recon.render_mesh(world["blob"][1], cams, size, shade, lighting=plain, **kw).image)


def test_lit_subject_with_transfer_in_the_scene(ops, recon, world):
    t = recon.Transfer(64)
    sh, direct, _ = params(3)
    lighting = recon.Lighting(sh, direct=direct, transfer=t)
    vol, bare = world["blob"]
    mesh = recon.with_transfer(bare, recon.mesh_transfer(bare, dev(vol), t)[0])
    scene, cam, size = world["scene"], cameras()[0], (48, 40)
    kw = dict(background=BG, **RASTER)
    got = recon.render_mesh_many_in_scene([mesh, None], scene, cam, size, "colors", lighting=lighting, **kw)
    unlit = recon.render_mesh_many_in_scene([mesh, None], scene, cam, size, "colors", **kw)
    front = recon.render_mesh(mesh, cam, size, "colors", lighting=lighting, **kw)
    uv = ops.mesh_render_raw(scene.verts, scene.faces, scene.counts, scene.attr, cam, size, background=BG, **RASTER)
    tex = scene_ref.texture(host(uv[0]), host(uv[2]), host(scene.pyramid), 64, 64, scene.levels, background=BG)
    want = scene_ref.composite([host(front.image)[None], host(front.depth)[None], host(front.face)[None]],
                               (tex, host(uv[1]), host(uv[2])), scene_ref.DEPTH, scene_ref.MIN_Z, BG)
    assert same(got[0].image, want[0][0]) and same(got[0].depth, want[1][0]) and same(got[0].mask, want[2][0])
    floor = host(got[0].mask) == 1
    assert floor.sum() > 20 and np.array_equal(bits(host(got[0].image))[floor], bits(host(unlit[0].image))[floor])
    for a, c in zip(got[1], unlit[1]):
        assert torch.equal(a.view(torch.uint8), c.view(torch.uint8))


# ---- the slots --------------------------------------------------------------------------------------------------------
TRANSFER_BUFFERS = ("transfer_bits", "transfer_prt", "transfer_shade", "light_ambient")


def traced(recon, slot, meshes, transfer):
    """The slot's own meshes with their transfer, traced by recon.mesh_transfer through the volume marching cubes read:
    with ``clean`` the cleaned one."""
    out = []
    for b, mesh in enumerate(meshes):
        if mesh is None:
            out.append(None)
            continue
        vol = slot.volumes[b]
        if slot.mesh.clean is not None:
            vol = recon.keep_largest(vol, slot.mesh.level, slot.mesh.clean)
        out.append(recon.with_transfer(mesh, recon.mesh_transfer(mesh, vol, transfer, slot.mesh.level, slot.b_min,
                                                                 slot.b_max)[0]))
    return out


def overflow(slot):
    """Run the slot's mesh chain and pictures again with capacities that frame 0 overflows."""
    for k, v in slot.mesh_buffers.items():
        slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
    with torch.cuda.stream(slot.stream):
        slot._mesh_chain(2)
        slot._render_pictures(2)
    slot._busy = True


def test_frame_slot_with_transfer_in_a_scene(recon, nets):  # noqa: F811
    """Clay, clean=6, a lit scene and the self-shadow: the slot == render_mesh_many_in_scene on its own meshes and their
    transfer; an empty frame; a forced overflow; and a slot whose lighting has no transfer."""
    from test_shadow_gpu import equal_pictures, slot_scene
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, frames, make_slot
    images, calibs = frames()
    scene = slot_scene(recon)
    t = recon.Transfer(64, reach=24)
    kw = dict(direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), albedo=(0.8, 0.7, 0.6), self_shadow=0.02)
    lighting, plain_lighting = recon.Lighting(params(4)[0], transfer=t, **kw), recon.Lighting(params(4)[0], **kw)
    opts = dict(SLOT_PICTURES, shade="normals", scene=scene)
    mesh = {"normals": "accumulate", "colors": False, "clean": 6}
    slot = make_slot(nets, mesh, opts, netc=False, lighting=lighting)
    plain = make_slot(nets, mesh, opts, netc=False, lighting=plain_lighting)
    try:
        r = slot.res[-1]
        assert tuple(slot.transfer_bits.shape) == (2, ref.bits_words(r)[1]) and slot.transfer_bits.dtype == torch.int32
        assert tuple(slot.transfer_prt.shape) == (2, 12 * r * r, 9) and tuple(slot.transfer_shade.shape) == (2, 12 * r * r, 3)
        assert tuple(slot.light_ambient.shape) == (2, 2) + SIZE + (3,)
        assert not any(hasattr(plain, k) for k in TRANSFER_BUFFERS)
        for s_ in (slot, plain):
            s_.submit(images, calibs, cameras=TWO)
            s_.wait()
        meshes, pics = slot.meshes(), slot.pictures()
        assert meshes[1] is None and all(isinstance(p, recon.ScenePicture) for p in pics)
        po = slot.picture_options
        args = (TWO, SIZE, "normals", po.projection, po.nearest, po.background, po.near, po.perspective_correct, "depth")
        own = traced(recon, slot, meshes, t)
        want = recon.render_mesh_many_in_scene(own, scene, *args, lighting=lighting)
        assert equal_pictures(pics[0], want[0]) and equal_pictures(pics[1], want[1])
        nv = meshes[0].verts.shape[0]
        assert torch.equal(slot.transfer_prt[0, :nv].view(torch.int32), own[0].transfer.view(torch.int32))
        # the bits are the cleaned volume's
        cleaned = recon.keep_largest(slot.volumes[0], 0.5, 6)
        fine = ref.bits_words(r)[0]
        assert np.array_equal(host(slot.transfer_bits[0])[:fine].view(np.uint32), ref.volume_bits(host(cleaned), 0.5))
        # the slot without transfer: the parent's bits, and other pixels on the subject only
        before = recon.render_mesh_many_in_scene(meshes, scene, *args, lighting=plain_lighting)
        base = plain.pictures()
        assert equal_pictures(base[0], before[0]) and equal_pictures(base[1], before[1])
        changed = (pics[0].image != base[0].image).any(-1)
        assert changed.sum() > 60 and (pics[0].mask[changed] == 2).all() and equal_pictures(pics[1], base[1])
        first = [p.clone() for p in pics[0]]
        overflow(slot)
        again = slot.pictures()
        assert slot._reran == [0] and int(again[1].mask.max()) == 1
        assert equal_pictures(again[0], first) and again[0].image.data_ptr() != slot.pictures_image[0].data_ptr()
    finally:
        slot.close()
        plain.close()


def test_views_slot_with_transfer(recon, views_net):  # noqa: F811
    """Clay, clean=6: the slot == render_mesh_many on its own meshes and their transfer; an empty frame; a forced
    overflow."""
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, bits_equal, make_views_slot
    images, calibs = views_frames()
    t = recon.Transfer(64, bias=1.0, step=0.5, reach=12)
    lighting = recon.Lighting(params(5)[0], direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), albedo=(0.8, 0.7, 0.6), transfer=t)
    mesh = {"normals": "accumulate", "colors": False, "clean": 6}
    slot = make_views_slot(views_net, mesh=mesh, pictures=dict(SLOT_PICTURES, shade="normals"), lighting=lighting)
    try:
        assert all(hasattr(slot, k) for k in TRANSFER_BUFFERS)
        slot.submit(images, calibs, cameras=TWO)
        meshes, pics = slot.meshes(), slot.pictures()
        assert meshes[1] is None and pics[1] is None
        po = slot.picture_options
        args = (TWO, SIZE, "normals", po.projection, po.nearest, po.background, po.near, po.perspective_correct)
        want = recon.render_mesh_many(traced(recon, slot, meshes, t), *args, lighting=lighting)
        assert all(bits_equal(a, b) for a, b in zip(pics[0], want[0])) and (pics[0].face >= 0).sum() > 60
        first = [p.clone() for p in pics[0]]
        overflow(slot)
        again = slot.pictures()
        assert slot._reran == [0] and again[1] is None and all(bits_equal(a, b) for a, b in zip(again[0], first))
    finally:
        slot.close()


def test_color_views_slot_with_transfer(recon, views_net, views_netc):  # noqa: F811
    """shade="netC", clean=6: the slot == render_mesh(shade="netC", lighting=) on its own mesh, maps and transfer; an
    empty frame; and a frame whose mesh overflowed is traced again through the slot's bits, coloured per pixel and lit
    again to the same bits."""
    t = recon.Transfer(128, reach=16)
    lighting = recon.Lighting(params(7)[0], direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), transfer=t)
    images, calibs = views_frames()
    cams = slot_cameras(2)
    mesh = {"normals": "accumulate", "colors": False, "clean": 6}
    slot = colour_slot(views_net, views_netc, mesh=mesh, pictures=dict(NETC_PICTURES, background=BG), lighting=lighting)
    bare = colour_slot(views_net, views_netc, mesh=mesh, pictures=dict(NETC_PICTURES, background=BG),
                       lighting=recon.Lighting(params(7)[0], direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7))))
    try:
        assert tuple(slot.light_ambient.shape) == (2, 2, 40, 24, 3) and slot.lighting is lighting
        assert not any(hasattr(bare, k) for k in TRANSFER_BUFFERS)
        for s_ in (slot, bare):
            s_.submit(images, calibs, cameras=cams)
        meshes, pics, base = slot.meshes(), slot.pictures(), bare.pictures()
        assert meshes[1] is None and pics[1] is None
        own = traced(recon, slot, meshes, t)
        nchw = torch.stack(own_maps(slot, 0)).permute(0, 3, 1, 2).contiguous()
        kw = dict(background=BG, netC=slot.netC, feat_tensor_C=[[nchw]], calib_tensor=slot.calib_in[0], view=slot.view)
        want = recon.render_mesh(own[0], cams[0], (40, 24), "netC", lighting=lighting, **kw)
        unoccluded = recon.render_mesh(meshes[0], cams[0], (40, 24), "netC", lighting=bare.lighting, **kw)
        assert int((want.face >= 0).sum()) >= 100 and not torch.equal(want.image, unoccluded.image)
        for a, w in zip(pics[0], want):
            assert a.dtype == w.dtype and torch.equal(a.view(torch.int32), w.view(torch.int32))
        for a, u in zip(base[0], unoccluded):
            assert torch.equal(a.view(torch.int32), u.view(torch.int32))
        nv = meshes[0].verts.shape[0]
        assert torch.equal(slot.transfer_prt[0, :nv].view(torch.int32), own[0].transfer.view(torch.int32))
        first = [p.clone() for p in pics[0]]
        overflow(slot)
        again = slot.pictures()
        assert slot._reran == [0] and again[1] is None and set(slot._reran_transfer) == {0}
        assert torch.equal(slot._reran_transfer[0][:nv].view(torch.int32), own[0].transfer.view(torch.int32))
        for a, b in zip(again[0], first):
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert again[0].image.data_ptr() != slot.pictures_image[0].data_ptr()
    finally:
        slot.close()
        bare.close()
