"""mp_picture_light / mp_picture_light_batch (csrc/light.hip), ops.picture_light_batch, recon.Lighting / light_picture,
``lighting=`` in render_mesh_many(_in_scene) and in a FrameSlot, on the GPU: every comparison is array_equal on the bits
against the numpy restatement (tests/light_ref.py, with shadow_ref.py / scene_ref.py for the shadow, the texture and
the composite), except the gamma step, which is held to a measured tolerance.  The rasteriser's pictures that the
restatements start from are the device's own: it has its bit-for-bit tests in test_mesh_render_gpu.py.
Needs an MI355X."""
import ctypes
import math

import numpy as np
import pytest

import light_ref as ref
import scene_ref
import shadow_cases
import shadow_ref
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

# powf under gamma = 2.2 against the float64 restatement on the f32 inputs of PICTURES, measured on one MI355X: the
# maximum absolute error of the shading (values between 0.5 and 4, so an ulp is 6e-8 .. 2.4e-7) was 2.05e-07 at 33 x 20
# and 2.51e-07 at 20 x 48, of the clamped image 1.17e-07 and 1.24e-07.  The bound is 4 x the largest of them, since
# powf's error varies with its argument.
GAMMA_MEASURED = 2.51e-07
GAMMA_TOL = 4 * GAMMA_MEASURED


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want):
    got = host(got) if torch.is_tensor(got) else got
    want = host(want) if torch.is_tensor(want) else want
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    return np.array_equal(bits(got), bits(want)) if got.dtype == F else np.array_equal(got, want)


def synthetic(size, seed=0):
    """Two views of a normal picture with uncovered spans longer than a wavefront, zero-length, NaN, inf, denormal and
    overflowing normals; an albedo with a NaN, a -0.0 and values outside [0, 1]; a visibility with exact 0 and 1."""
    rng = np.random.RandomState(seed)
    h, w = size
    normal = (rng.standard_normal((2, h, w, 3)) * rng.uniform(0.1, 3.0, (2, h, w, 1))).astype(F)
    flat = normal.reshape(-1, 3)
    flat[5] = [0.0, 0.0, 0.0]
    flat[6] = [np.nan, 0.5, 0.5]
    flat[7] = [0.3, np.inf, 0.1]
    flat[8] = [-0.0, -0.0, 0.0]
    flat[9] = [1e-30, 0.0, 0.0]   # the squared length underflows to 0
    flat[10] = [3e19, 3e19, 0.0]  # and here it overflows
    flat[11] = [1e-20, 2e-20, 1e-20]  # a denormal squared length
    flat[12] = [0.0, 0.0, -2.0]
    face = rng.randint(0, 50, (2, h, w)).astype(np.int32)
    face.reshape(-1)[100:300] = -1
    face.reshape(-1)[h * w + 17:h * w + 17 + 130] = -1
    face[rng.rand(2, h, w) < 0.1] = -1
    face.reshape(-1)[5:13] = 3
    albedo = rng.uniform(-0.2, 1.4, (2, h, w, 3)).astype(F)
    albedo.reshape(-1, 3)[3] = [np.nan, -0.0, np.inf]
    albedo.reshape(-1, 3)[150] = [np.nan, -0.0, -np.inf]  # uncovered: its bits travel
    vis = rng.uniform(0.0, 1.0, (2, h, w)).astype(F)
    vis.reshape(-1)[20:40] = 0.0
    vis.reshape(-1)[40:60] = 1.0
    return normal, face, albedo, vis


def params(seed=0):
    rng = np.random.RandomState(100 + seed)
    sh = rng.uniform(-0.6, 0.9, (9, 3)).astype(F)
    d = rng.standard_normal(3)
    direct = ((d / np.linalg.norm(d)).astype(F), rng.uniform(0.2, 1.0, 3).astype(F))
    mats = rng.standard_normal((2, 3, 3)).astype(F)
    return sh, direct, mats


@pytest.mark.parametrize("size", PICTURES, ids=lambda s: "%dx%d" % s)
def test_kernel_against_the_restatement(ops, size):
    normal, face, albedo, vis = synthetic(size)
    sh, direct, mats = params()
    d_normal, d_face, d_albedo, d_vis = (dev(a) for a in (normal, face, albedo, vis))
    rgb = (0.8, 0.7, 0.6)
    lit = 0
    for with_mats in (False, True):
        for with_direct in (False, True):
            for with_vis in (False, True):
                for constant in (False, True):
                    what = (with_mats, with_direct, with_vis, constant)
                    want_image, want_shading = ref.light(
                        normal, face, None if constant else albedo, sh, *(direct if with_direct else (None, None)),
                        normal_mats=mats if with_mats else None, n_views=2, visibility=vis if with_vis else None,
                        albedo_rgb=rgb if constant else None, background=BG)
                    want_image, want_shading = want_image.reshape(albedo.shape), want_shading.reshape(albedo.shape)
                    lit += int((want_image != (BG if constant else albedo)).sum())
                    kw = dict(direct=direct if with_direct else None, normal_mats=mats if with_mats else None,
                              visibilities=[d_vis] if with_vis else None, albedo_rgb=rgb if constant else None,
                              background=BG)
                    alb = None if constant else [d_albedo]
                    got = ops.picture_light_batch([d_normal], [d_face], alb, sh, with_shading=True, **kw)[0]
                    assert same(got[0], want_image) and same(got[1], want_shading), what
                    shading = torch.empty_like(d_normal)  # the shading alone
                    got = ops.picture_light_batch([d_normal], [d_face], alb, sh, out=(None, [shading]), **kw)[0]
                    assert got[0] is None and got[1] is shading and same(shading, want_shading), what
                    got = ops.picture_light_batch([d_normal], [d_face], alb, sh, **kw)[0]  # the image alone
                    assert got[1] is None and same(got[0], want_image), what
                    if not constant:  # in place
                        own = d_albedo.clone()
                        got = ops.picture_light_batch([d_normal], [d_face], [own], sh, out=([own], None), **kw)[0]
                        assert got[0] is own and same(own, want_image), what
    assert lit > 1000
    assert same(d_albedo, albedo) and same(d_normal, normal)  # out of place: the inputs are not written


def test_the_degenerate_normals_are_what_the_definition_says(ops):
    """Zero, NaN, inf, underflowing and overflowing normals shade as the normal (0, 0, 0): the constant and H6's -c5."""
    normal, face, albedo, vis = synthetic((33, 20))
    sh, direct, _ = params()
    got = ops.picture_light_batch([dev(normal)], [dev(face)], None, sh, direct=direct, albedo_rgb=(1, 1, 1),
                                  with_shading=True)[0][1]
    flat = host(got).reshape(-1, 3)
    res = np.zeros(3, F)  # H = (c4, 0, 0, 0, 0, 0, -c5, 0, 0); the direct term adds 0 * rgb
    for i, h in enumerate([F(0.886227), F(0), F(0), F(0), F(0), F(0), F(0) - F(0.247708), F(0), F(0)]):
        res = res + h * sh[i]
    assert res.dtype == F
    for p in (5, 6, 7, 8, 9, 10):
        assert np.array_equal(bits(flat[p]), bits(res)), p
    assert not np.array_equal(flat[11], res) and not np.array_equal(flat[12], res)  # short and long normals are normals


def test_batched_equals_per_frame(ops):
    """Three frames in one launch against mp_picture_light on each, with matrices per frame and view."""
    size = (20, 48)
    frames = [synthetic(size, seed) for seed in (1, 2, 3)]
    sh, direct, _ = params(1)
    mats = np.stack([params(s)[2] for s in (1, 2, 3)])
    d = [[dev(a) for a in fr] for fr in frames]
    got = ops.picture_light_batch([f[0] for f in d], [f[1] for f in d], [f[2] for f in d], sh, direct=direct,
                                  normal_mats=mats, visibilities=[f[3] for f in d], with_shading=True)
    ctx = ops.get_context(DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    n = frames[0][1].size
    for f in range(3):
        normal, face, albedo, vis = frames[f]
        want = ref.light(normal, face, albedo, sh, *direct, normal_mats=mats[f], n_views=2, visibility=vis)
        assert same(got[f][0], want[0].reshape(albedo.shape)) and same(got[f][1], want[1].reshape(albedo.shape)), f
        image, shading = torch.empty_like(d[f][2]), torch.empty_like(d[f][2])
        m = np.ascontiguousarray(mats[f])
        rc = ctx.lib.mp_picture_light(ctx.handle, d[f][0].data_ptr(), d[f][1].data_ptr(), d[f][2].data_ptr(), None,
                                      d[f][3].data_ptr(), n, 2, sh.ctypes.data_as(PF), direct[0].ctypes.data_as(PF),
                                      direct[1].ctypes.data_as(PF), 1.0, m.ctypes.data_as(PF), 1.0, image.data_ptr(),
                                      shading.data_ptr(), stream)
        assert rc == OK and same(image, got[f][0]) and same(shading, got[f][1]), f
    assert not same(got[0][1], got[1][1])


def test_more_views_than_a_call_holds_matrices(ops):
    """40 views of 3 x 5 pixels with a matrix each: the wrapper splits the views; the same bits as the restatement."""
    rng = np.random.RandomState(5)
    normal = rng.standard_normal((40, 3, 5, 3)).astype(F)
    face = np.where(rng.rand(40, 3, 5) < 0.8, 1, -1).astype(np.int32)
    albedo = rng.uniform(0, 1, (40, 3, 5, 3)).astype(F)
    sh, direct, _ = params(2)
    mats = rng.standard_normal((40, 3, 3)).astype(F)
    got = ops.picture_light_batch([dev(normal)] * 2, [dev(face)] * 2, [dev(albedo)] * 2, sh, direct=direct,
                                  normal_mats=mats, with_shading=True)
    want = ref.light(normal, face, albedo, sh, *direct, normal_mats=mats, n_views=40)
    for f in range(2):
        assert same(got[f][0], want[0].reshape(albedo.shape)) and same(got[f][1], want[1].reshape(albedo.shape))


@pytest.mark.parametrize("size", PICTURES, ids=lambda s: "%dx%d" % s)
def test_gamma_against_float64(ops, size):
    normal, face, albedo, vis = synthetic(size)
    sh, direct, mats = params()
    # shadings well above 0, where the power's slope is bounded: a large constant term, small others (asserted below)
    sh = np.abs(sh) * F(0.3)
    sh[0] += F(2.0)
    face = face.copy()
    face.reshape(-1)[9:12] = -1  # squared lengths that leave f32's range are in range in float64: another normal there
    got = ops.picture_light_batch([dev(normal)], [dev(face)], [dev(albedo)], sh, direct=direct, gamma=2.2,
                                  normal_mats=mats, visibilities=[dev(vis)], with_shading=True)[0]
    want = ref.light(normal, face, albedo, sh, *direct, gamma=2.2, normal_mats=mats, n_views=2, visibility=vis,
                     dtype=np.float64)
    image, shading = host(got[0]).reshape(-1, 3).astype(np.float64), host(got[1]).reshape(-1, 3).astype(np.float64)
    cov = face.reshape(-1) >= 0
    ok = np.isfinite(want[0]).all(1) & cov
    assert ok.sum() > 0.7 * cov.sum()
    err_shading = float(np.abs(shading[cov] - want[1][cov]).max())
    err_image = float(np.abs(image[ok] - want[0][ok]).max())
    print("gamma 2.2, %dx%d: max |shading - f64| = %.3e, max |image - f64| = %.3e" % (size + (err_shading, err_image)))
    assert float(want[1][cov].min()) > 0.5 and float(want[1][cov].max()) < 4.0
    assert err_shading <= GAMMA_TOL and err_image <= GAMMA_TOL
    uncovered = ~cov
    assert np.array_equal(bits(host(got[0]).reshape(-1, 3)[uncovered]), bits(albedo.reshape(-1, 3)[uncovered]))
    assert not host(got[1]).reshape(-1, 3)[uncovered].any()


# ---- refusals -------------------------------------------------------------------------------------------------------
class Env:
    """A well-formed call of mp_picture_light on small real buffers; every refusal changes one argument."""

    def __init__(self, ops):
        self.ctx = ops.get_context(DEV)
        self.lib = self.ctx.lib
        z = lambda *s, **k: torch.zeros(*s, device=DEV, **k)  # noqa: E731
        self.n = 24
        self.normal, self.albedo, self.out, self.shading, self.vis = z(24, 3), z(24, 3), z(24, 3), z(24, 3), z(24)
        self.face = z(24, dtype=torch.int32)
        self.normal[:, 2] = 1.0
        self.sh = np.zeros((9, 3), F)  # the direct light alone, head on: the shading is its rgb exactly
        self.dir, self.rgb, self.const = np.array([0, 0, -1], F), np.full(3, 0.5, F), np.ones(3, F)
        self.mats = np.tile(np.eye(3, dtype=F), (2, 1, 1))
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)

    def done(self, rc):
        return rc, self.lib.mp_last_error(self.ctx.handle).decode()

    @staticmethod
    def pf(a):
        return PF() if a is None else a.ctypes.data_as(PF)

    def light(self, **k):
        a = dict(normal=self.normal.data_ptr(), face=self.face.data_ptr(), albedo=self.albedo.data_ptr(), const=None,
                 vis=self.vis.data_ptr(), n=self.n, views=2, sh=self.sh, dir=self.dir, rgb=self.rgb, gamma=1.0,
                 mats=self.mats, background=1.0, out=self.out.data_ptr(), shading=self.shading.data_ptr())
        a.update(k)
        return self.done(self.lib.mp_picture_light(
            self.ctx.handle, a["normal"], a["face"], a["albedo"], self.pf(a["const"]), a["vis"], a["n"], a["views"],
            self.pf(a["sh"]), self.pf(a["dir"]), self.pf(a["rgb"]), a["gamma"], self.pf(a["mats"]), a["background"],
            a["out"], a["shading"], self.stream))


def test_refusals_through_the_c_abi(ops):
    env = Env(ops)
    env.albedo.fill_(0.5)
    assert env.light()[0] == OK
    assert env.light(out=env.albedo.data_ptr(), shading=None)[0] == OK   # in place
    assert env.light(albedo=None, const=env.const, out=None)[0] == OK    # the shading alone, a constant albedo
    assert env.light(vis=None, mats=None, gamma=2.2, shading=None)[0] == OK
    torch.cuda.synchronize()
    assert (env.albedo == 0.25).all() and (env.shading == 0.5).all()
    bad = lambda a, i: np.where(np.arange(a.size).reshape(a.shape) == i, F(np.nan), a).astype(F)  # noqa: E731
    refused = [
        (dict(n=0), ARG, "n_pixels"),
        (dict(n=0x7fffffff // 3 + 1), UNSUPPORTED, "2^31 / 3"),
        (dict(views=0), ARG, "n_views"),
        (dict(views=5), ARG, "n_views"),
        (dict(n=33, views=33, mats=np.tile(np.eye(3, dtype=F), (33, 1, 1))), ARG, "normal matrices"),
        (dict(sh=None), ARG, "bad argument"),
        (dict(dir=None), ARG, "bad argument"),
        (dict(rgb=None), ARG, "bad argument"),
        (dict(const=env.const), ARG, "both"),
        (dict(albedo=None), ARG, "neither"),
        (dict(gamma=0.0), ARG, "gamma"),
        (dict(gamma=-2.2), ARG, "gamma"),
        (dict(gamma=math.nan), ARG, "gamma"),
        (dict(gamma=math.inf), ARG, "gamma"),
        (dict(sh=bad(env.sh, 26)), ARG, "finite"),
        (dict(dir=bad(env.dir, 1)), ARG, "finite"),
        (dict(rgb=np.array([0, np.inf, 0], F)), ARG, "finite"),
        (dict(albedo=None, const=bad(env.const, 2)), ARG, "finite"),
        (dict(mats=bad(env.mats, 17)), ARG, "finite"),
        (dict(background=math.nan), ARG, "finite"),
        (dict(out=None, shading=None), ARG, "no output"),
        (dict(normal=None), ARG, "null"),
        (dict(face=None), ARG, "null"),
        (dict(normal=env.normal.data_ptr() + 2), ARG, "misaligned"),
        (dict(vis=env.vis.data_ptr() + 1), ARG, "misaligned"),
        (dict(out=env.albedo.data_ptr() + 12), ARG, "aliases"),          # the albedo shifted by a pixel
        (dict(out=env.normal.data_ptr()), ARG, "aliases"),
        (dict(shading=env.albedo.data_ptr()), ARG, "aliases"),
        (dict(shading=env.face.data_ptr(), n=6, views=1), ARG, "aliases"),
        (dict(out=env.vis.data_ptr(), n=6, views=1), ARG, "aliases"),
        (dict(shading=env.out.data_ptr()), ARG, "aliases"),
    ]
    for t in (env.out, env.shading, env.albedo):
        t.fill_(5.0)
    for changed, code, word in refused:
        rc, msg = env.light(**changed)
        assert rc == code and msg.startswith("mp_picture_light:") and word in msg, (changed, rc, msg)
    torch.cuda.synchronize()
    assert (env.out == 5.0).all() and (env.shading == 5.0).all() and (env.albedo == 5.0).all()  # nothing was launched
    # the batched form carries its own name and refuses a frame count out of range
    ptr = (ctypes.c_void_p * 1)(env.normal.data_ptr())
    for n_frames in (0, 33):
        rc = env.lib.mp_picture_light_batch(env.ctx.handle, n_frames, ptr, ptr, ptr, PF(), ptr, 24, 2, env.pf(env.sh),
                                            env.pf(env.dir), env.pf(env.rgb), 1.0, PF(), 1.0, ptr, ptr, env.stream)
        assert env.done(rc)[0] == ARG and env.done(rc)[1].startswith("mp_picture_light_batch:")


def test_cross_frame_aliasing_is_refused(ops):
    """The batched call: an output of frame f may share no byte with an input or an output of another frame; in place is
    image_out[f] == albedo[f] only."""
    env = Env(ops)
    z = lambda *s_, **k: torch.zeros(*s_, device=DEV, **k)  # noqa: E731
    normal, albedo, out, shading = ([z(24, 3), z(24, 3)] for _ in range(4))
    face, vis = [z(24, dtype=torch.int32) for _ in range(2)], [z(24), z(24)]
    arr = lambda ts: (ctypes.c_void_p * 2)(*[t.data_ptr() for t in ts])  # noqa: E731

    def call(**k):
        a = dict(normal=normal, face=face, albedo=albedo, vis=vis, out=out, shading=shading)
        a.update(k)
        return env.done(env.lib.mp_picture_light_batch(
            env.ctx.handle, 2, arr(a["normal"]), arr(a["face"]), arr(a["albedo"]), PF(), arr(a["vis"]), 24, 2,
            env.pf(env.sh), env.pf(env.dir), env.pf(env.rgb), 1.0, env.pf(np.tile(env.mats, (2, 1, 1))), 1.0,
            None if a["out"] is None else arr(a["out"]), None if a["shading"] is None else arr(a["shading"]), env.stream))

    for t in albedo:
        t.fill_(0.5)
    for t in normal:
        t[:, 2] = 1.0
    assert call()[0] == OK and call(out=albedo, shading=None)[0] == OK  # in place, both frames
    torch.cuda.synchronize()
    assert all((t == 0.25).all() for t in albedo) and all((t == 0.5).all() for t in shading)
    for t in albedo + out + shading:
        t.fill_(5.0)
    refused = [
        (dict(out=albedo[::-1]), "input"),                       # image_out[0] == albedo[1]: not in place
        (dict(out=[out[0], albedo[0]]), "input"),                # image_out[1] == albedo[0]
        (dict(shading=[shading[0], normal[0]]), "input"),        # shading[1] == normal[0]
        (dict(out=[out[0], out[0]]), "output"),                  # the two frames write one image
        (dict(shading=[shading[1], shading[1]]), "output"),
        (dict(out=[out[0], shading[0]]), "output"),              # image_out[1] == shading[0]
        (dict(out=[out[0], out[0][1:]]), "output"),              # shifted by a pixel
    ]
    for changed, word in refused:
        rc, msg = call(**changed)
        assert rc == ARG and msg.startswith("mp_picture_light_batch:") and "aliases an " + word in msg, (changed, rc, msg)
    torch.cuda.synchronize()
    assert all((t == 5.0).all() for t in albedo + out + shading)  # nothing was launched


def test_gamma_of_a_negative_shading_is_zero(ops):
    """max0 in front of powf: a negative (and a -0.0) shading gives +0.0 under a gamma, not a NaN."""
    normal = np.tile(np.array([0, 0, 1], F), (2, 5, 1))
    face = np.zeros((2, 5), np.int32)
    sh = np.zeros((9, 3), F)
    direct = (np.array([0, 0, -1], F), np.array([-0.5, 0.25, 4.0], F))
    for vis, want in ((None, [0.0, 0.25 ** (1 / 2.2), 4.0 ** (1 / 2.2)]), (np.ones((2, 5), F), [0.0, 0.0, 0.0])):
        got = ops.picture_light_batch([dev(normal)], [dev(face)], None, sh, direct=direct, gamma=2.2, albedo_rgb=(1, 1, 1),
                                      visibilities=None if vis is None else [dev(vis)], with_shading=True)[0]
        shading, image = host(got[1]).reshape(-1, 3), host(got[0]).reshape(-1, 3)
        assert np.isfinite(shading).all() and not np.signbit(shading).any()
        assert np.array_equal(bits(shading[:, 0]), bits(np.zeros(10, F))) and np.array_equal(shading, shading[:1].repeat(10, 0))
        assert np.abs(shading[0].astype(np.float64) - want).max() <= GAMMA_TOL
        assert np.array_equal(image, np.minimum(shading, F(1)))
        ref_image, ref_shading = ref.light(normal, face, None, sh, *direct, gamma=2.2, visibility=vis, albedo_rgb=(1, 1, 1))
        assert np.array_equal(bits(ref_shading[:, 0]), bits(shading[:, 0]))


def test_ops_refuses_before_it_enqueues(ops):
    normal, face, albedo, vis = [dev(a) for a in synthetic((33, 20))]
    sh, direct, mats = params()
    call = lambda **k: ops.picture_light_batch([normal], [face], k.pop("albedos", [albedo]), k.pop("sh", sh), **k)  # noqa: E731
    for kw in (dict(gamma=0.0), dict(gamma=math.nan), dict(gamma="2.2"), dict(sh=sh[:8]), dict(sh=np.full((9, 3), np.nan)),
               dict(direct=(direct[0],)), dict(direct=((0, np.inf, 0), (1, 1, 1))), dict(albedo_rgb=(1, 1, 1)),
               dict(albedos=None), dict(albedos=None, albedo_rgb=(1, 1)), dict(normal_mats=mats[:1]),
               dict(normal_mats=mats * np.nan), dict(n_views=7), dict(n_views=0), dict(background=math.inf),
               dict(out=(None, None)), dict(out=([normal], None)), dict(visibilities=[vis.double()]),
               dict(out=([albedo], [albedo]))):
        with pytest.raises((ValueError, RuntimeError)):
            call(**kw)


# ---- the whole path with the real rasteriser: the shadow test's sphere over its floor ---------------------------------
NEAR = 3.4  # cuts the sphere's near cap: the subject's picture is the clipped one


def cameras():
    """Two perspective cameras above the floor, tilted down at it: [2,4,4] float32."""
    out = []
    for a, tx in ((-0.6, -0.3), (-0.3, 0.2)):
        c, s = math.cos(a), math.sin(a)
        m = np.eye(4)
        m[:3, :3] = np.diag([1.2, 1.2, 1.0]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
        m[:3, 3] = [tx, 0.0, 4.0]
        out.append(m.astype(F))
    return torch.from_numpy(np.stack(out))


@pytest.fixture(scope="module")
def world(recon):
    from monoport_amd import mesh_util
    verts, faces = shadow_cases.sphere_mesh()
    normals = np.ascontiguousarray(mesh_util.compute_normal(verts, faces, "accumulate"), F)
    mesh = recon.Mesh(dev(verts), dev(faces), dev(normals), dev((verts * F(0.4) + F(0.5)).astype(F)))
    fv, ff, uv = shadow_cases.plank(x=(-2.0, 3.0), z=(-1.5, 1.5))
    light = shadow_cases.light(recon, radius=1, strength=0.6)
    return dict(mesh=mesh, light=light, lit=recon.Scene(fv, ff, uv, procedural(64, 64), device=DEV, light=light),
                dark=recon.Scene(fv, ff, uv, procedural(64, 64), device=DEV))


def lighting_of(recon, **kw):
    sh, _, _ = params(3)
    return recon.Lighting(sh, direct=(shadow_cases.DIRECTION, (0.9, 0.8, 0.7)), **kw)


RASTER = dict(projection="perspective", nearest="min", near=NEAR, perspective_correct=True)


def mesh_counts(mesh):
    return torch.tensor([mesh.verts.shape[0], mesh.faces.shape[0]], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("frame", ["world", "camera"])
@pytest.mark.parametrize("shade", ["colors", "normals"])
def test_lit_pictures_against_the_restatement(ops, recon, world, shade, frame):
    mesh, cams, size = world["mesh"], cameras(), (33, 20)
    lighting = lighting_of(recon, frame=frame, albedo=(0.8, 0.7, 0.6) if shade == "normals" else None)
    kw = dict(background=BG, **RASTER)
    got = recon.render_mesh_many([mesh, None], cams, size, shade, lighting=lighting, **kw)
    assert got[1] is None
    front = recon.render_mesh(mesh, cams, size, shade, **kw)
    nrm = ops.mesh_render_raw(mesh.verts, mesh.faces, mesh_counts(mesh), mesh.normals, cams, size, background=BG, **RASTER)
    assert torch.equal(nrm[2], front.face) and (front.face >= 0).sum() > 30  # the second pass sees the first one's faces
    mats = host(cams)[:, :3, :3] if frame == "camera" else None
    want_image, want_shading = ref.light(host(nrm[0]), host(nrm[2]), None if shade == "normals" else host(front.image),
                                         lighting.sh, lighting.direct_dir, lighting.direct_rgb, normal_mats=mats,
                                         n_views=2, albedo_rgb=lighting.albedo, background=BG)
    assert same(got[0].image, want_image.reshape(2, *size, 3))
    assert torch.equal(got[0].face, front.face) and same(got[0].depth, front.depth)
    assert not same(got[0].image, front.image)
    # one camera, and the generic call on the pieces
    single = recon.render_mesh(mesh, cams[1], size, shade, lighting=lighting, **kw)
    assert same(single.image, want_image.reshape(2, *size, 3)[1])
    image, shading = recon.light_picture((None if shade == "normals" else front.image, front.depth, front.face), nrm[0],
                                         lighting, calibs=cams)
    assert same(shading, want_shading.reshape(2, *size, 3))
    if shade == "colors":  # light_picture without an image writes 1.0 where nothing is covered, the render BG
        assert same(image, want_image.reshape(2, *size, 3))
    # a second run gives the same bits
    again = recon.render_mesh_many([mesh, None], cams, size, shade, lighting=lighting, **kw)
    assert same(again[0].image, got[0].image)


def test_lit_subject_with_self_shadow_in_the_lit_scene(ops, recon, world):
    mesh, light, lit = world["mesh"], world["light"], world["lit"]
    cam, size, bias = cameras()[0], (64, 64), 0.05
    lighting = lighting_of(recon, self_shadow=bias)
    plain = lighting_of(recon)
    kw = dict(background=BG, **RASTER)
    got = recon.render_mesh_many_in_scene([mesh, None], lit, cam, size, "colors", lighting=lighting, **kw)
    unshadowed = recon.render_mesh_many_in_scene([mesh, None], lit, cam, size, "colors", lighting=plain, **kw)
    unlit = recon.render_mesh_many_in_scene([mesh, None], lit, cam, size, "colors", **kw)
    # the pieces: the subject's colours, normals and positions, the shadow map, its own shade
    front = recon.render_mesh(mesh, cam, size, "colors", **kw)
    counts = mesh_counts(mesh)
    nrm = ops.mesh_render_raw(mesh.verts, mesh.faces, counts, mesh.normals, cam, size, background=BG, **RASTER)
    pos = ops.mesh_render_raw(mesh.verts, mesh.faces, counts, mesh.verts, cam, size, background=BG, **RASTER)
    assert torch.equal(nrm[2][0], front.face) and torch.equal(pos[2][0], front.face)
    smap = ops.mesh_render_raw(mesh.verts, mesh.faces, counts, None, light.calib, light.res, "orthogonal", "min")
    vis = shadow_ref.shade(host(pos[0]), host(pos[2]), host(smap[1])[0], host(smap[2])[0], light.calib,
                           shadow_ref.ORTHOGONAL, shadow_ref.MIN_Z, bias, light.radius)
    covered = host(front.face) >= 0
    assert (vis[0][covered] == 1.0).sum() > 5 and (vis[0][covered] == 0.0).sum() > 5  # a lit and a dark side
    want_front, _ = ref.light(host(nrm[0]), host(nrm[2]), host(front.image), lighting.sh, lighting.direct_dir,
                              lighting.direct_rgb, visibility=vis, background=BG)
    want_front = want_front.reshape(1, *size, 3)
    # the scene, as test_shadow_gpu.py composes it
    uv = ops.mesh_render_raw(lit.verts, lit.faces, lit.counts, lit.attr, cam, size, background=BG, **RASTER)
    spos = ops.mesh_render_raw(lit.verts, lit.faces, lit.counts, lit.verts, cam, size, background=BG, **RASTER)
    tex = scene_ref.texture(host(uv[0]), host(uv[2]), host(lit.pyramid), 64, 64, lit.levels, background=BG)
    want_back, _ = shadow_ref.shadow(tex, host(spos[0]), host(uv[2]), host(smap[1])[0], host(smap[2])[0], light.calib,
                                     shadow_ref.ORTHOGONAL, shadow_ref.MIN_Z, light.bias, light.radius, light.strength)
    want = scene_ref.composite([want_front, host(front.depth)[None], host(front.face)[None]],
                               (want_back, host(uv[1]), host(uv[2])), scene_ref.DEPTH, scene_ref.MIN_Z, BG)
    assert same(got[0].image, want[0][0]) and same(got[0].depth, want[1][0]) and same(got[0].mask, want[2][0])
    assert torch.equal(got[0].face, front.face)
    # the scene keeps its texture and its shadow; the self-shadow darkens the subject only, and only where vis > 0
    subject, floor = host(got[0].mask) == 2, host(got[0].mask) == 1
    assert np.array_equal(bits(host(got[0].image))[floor], bits(host(unlit[0].image))[floor]) and floor.sum() > 20
    darker = (host(got[0].image) < host(unshadowed[0].image)).any(-1)
    assert (darker & subject).sum() > 5 and not (darker & ~subject).any() and not (darker & (vis[0] == 0)).any()
    assert not (host(got[0].image) > host(unshadowed[0].image)).any()
    # no mesh: the bare scene, the bits of the call without lighting
    for a, c in zip(got[1], unlit[1]):
        assert torch.equal(a.view(torch.uint8), c.view(torch.uint8))


# ---- the slots ------------------------------------------------------------------------------------------------------
LIGHT_BUFFERS = ("light_normal", "light_face", "light_pos", "light_shade")


def test_frame_slot_clay_with_self_shadow_in_a_lit_scene(recon, nets):  # noqa: F811
    from test_shadow_gpu import equal_pictures, slot_scene
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, frames, make_slot
    images, calibs = frames()
    scene = slot_scene(recon)
    lighting = recon.Lighting(params(4)[0], direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), frame="camera",
                              albedo=(0.8, 0.7, 0.6), self_shadow=0.02)
    opts = dict(SLOT_PICTURES, shade="normals", scene=scene)
    mesh = {"normals": "accumulate", "colors": False}
    slot = make_slot(nets, mesh, opts, netc=False, lighting=lighting)
    plain = make_slot(nets, mesh, opts, netc=False)
    none = make_slot(nets, mesh, opts, netc=False, lighting=None)
    try:
        assert tuple(slot.light_normal.shape) == tuple(slot.light_pos.shape) == (2, 2) + SIZE + (3,)
        assert tuple(slot.light_face.shape) == tuple(slot.light_shade.shape) == (2, 2) + SIZE
        assert slot.light_face.dtype == torch.int32 and slot.lighting is lighting
        for s in (plain, none):
            assert s.lighting is None and not any(hasattr(s, k) for k in LIGHT_BUFFERS)
        for s in (slot, plain, none):
            s.submit(images, calibs, cameras=TWO)
            s.wait()
        meshes, pics = slot.meshes(), slot.pictures()
        assert meshes[1] is None and all(isinstance(p, recon.ScenePicture) for p in pics)
        po = slot.picture_options
        args = (TWO, SIZE, "normals", po.projection, po.nearest, po.background, po.near, po.perspective_correct, "depth")
        want = recon.render_mesh_many_in_scene(meshes, scene, *args, lighting=lighting)
        assert equal_pictures(pics[0], want[0]) and equal_pictures(pics[1], want[1])
        assert pics[0].image.data_ptr() == slot.pictures_image[0].data_ptr()
        assert torch.equal(slot.light_face[0], slot.pictures_face[0])  # the normal pass saw the first pass's faces
        assert (slot.light_shade[0] == 1.0).any() and (slot.light_shade[0] == 0.0).any()
        # the slot built with lighting=None: the bits of the slot built without the keyword, which are today's
        before = recon.render_mesh_many_in_scene(meshes, scene, *args)
        for p, q in zip(plain.pictures(), none.pictures()):
            assert equal_pictures(p, q)
        assert equal_pictures(plain.pictures()[0], before[0]) and equal_pictures(plain.pictures()[1], before[1])
        # lighting changes the subject's pixels only; the empty frame is the bare (shadowless) scene
        changed = (pics[0].image != before[0].image).any(-1)
        assert changed.sum() > 60 and (pics[0].mask[changed] == 2).all()
        assert equal_pictures(pics[1], before[1]) and int(pics[1].mask.max()) == 1 and (slot.light_face[1] == -1).all()
        # a frame whose mesh overflowed the slot's capacities: rendered, lit, shadowed and composited again, the same bits
        first = [t.clone() for t in pics[0]]
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
            slot._render_pictures(2)
        slot._busy = True
        again = slot.pictures()
        assert slot._reran == [0] and int(again[1].mask.max()) == 1
        assert equal_pictures(again[0], first) and again[0].image.data_ptr() != slot.pictures_image[0].data_ptr()
    finally:
        slot.close()
        plain.close()
        none.close()


def test_frame_slot_lit_netc_pictures(ops, recon, nets):  # noqa: F811
    """shade="netC" without a scene: the slot's picture is the lighting of the unlit slot's picture at the normals of
    its own mesh; and the slot with a constant albedo and no netC equals render_mesh_many, also after an overflow."""
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, bits_equal, frames, make_slot
    images, calibs = frames()
    lighting = recon.Lighting(params(5)[0], direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)))
    clay = recon.Lighting(params(5)[0], albedo=(0.8, 0.7, 0.6), frame="camera")
    mesh = {"normals": "accumulate", "colors": False}
    slot = make_slot(nets, mesh, dict(SLOT_PICTURES, shade="netC"), lighting=lighting)
    plain = make_slot(nets, mesh, dict(SLOT_PICTURES, shade="netC"))
    solid = make_slot(nets, mesh, dict(SLOT_PICTURES, shade="normals"), netc=False, lighting=clay)
    try:
        assert not hasattr(slot, "light_pos") and not hasattr(slot, "light_shade") and not hasattr(plain, "light_normal")
        for s in (slot, plain, solid):
            s.submit(images, calibs, cameras=TWO)
        pics, base, meshes = slot.pictures(), plain.pictures(), slot.meshes()
        assert pics[1] is None and base[1] is None and meshes[1] is None
        po = slot.picture_options
        raster = dict(projection=po.projection, nearest=po.nearest, near=po.near, perspective_correct=po.perspective_correct)
        m = meshes[0]
        nrm = ops.mesh_render_raw(m.verts.contiguous(), m.faces.contiguous(), mesh_counts(m), m.normals.contiguous(), TWO,
                                  SIZE, background=po.background, **raster)
        assert torch.equal(nrm[2], base[0].face) and torch.equal(slot.light_face[0], base[0].face)
        want = recon.light_picture(base[0], nrm[0], lighting)[0]
        assert bits_equal(pics[0].image, want) and not bits_equal(pics[0].image, base[0].image)
        # and render_mesh_many(shade="netC", lighting=) on the slot's own mesh, maps and calibration
        nchw = slot.feats_hwc_c[0].permute(2, 0, 1)[None].contiguous()
        many = recon.render_mesh_many(meshes, TWO, SIZE, "netC", po.projection, po.nearest, po.background, po.near,
                                      po.perspective_correct, netC=slot.netC, feat_tensors_C=[[[nchw]], None],
                                      calib_tensors=[slot.calib[0:1], None], lighting=lighting)
        assert many[1] is None and all(bits_equal(a, b) for a, b in zip(pics[0], many[0]))
        assert bits_equal(pics[0].depth, base[0].depth) and torch.equal(pics[0].face, base[0].face)
        uncovered = base[0].face < 0
        assert (pics[0].image[uncovered] == po.background).all() and uncovered.any()
        # the clay slot against render_mesh_many on its own meshes, then after a forced overflow
        args = (TWO, SIZE, "normals", po.projection, po.nearest, po.background, po.near, po.perspective_correct)
        got, own = solid.pictures(), solid.meshes()
        want = recon.render_mesh_many(own, *args, lighting=clay)
        assert got[1] is None and want[1] is None
        assert all(bits_equal(a, b) for a, b in zip(got[0], want[0]))
        first = [t.clone() for t in got[0]]
        for k, v in solid.mesh_buffers.items():
            solid.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(solid.stream):
            solid._mesh_chain(2)
            solid._render_pictures(2)
        solid._busy = True
        again = solid.pictures()
        assert solid._reran == [0] and all(bits_equal(a, b) for a, b in zip(again[0], first))
        assert again[0].image.data_ptr() != solid.pictures_image[0].data_ptr()
        # the same for the netC slot: the re-run mesh is coloured per pixel and lit again, the same bits
        first = [t.clone() for t in pics[0]]
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
            slot._render_pictures(2)
        slot._busy = True
        again = slot.pictures()
        assert slot._reran == [0] and again[1] is None and all(bits_equal(a, b) for a, b in zip(again[0], first))
        assert again[0].image.data_ptr() != slot.pictures_image[0].data_ptr()
    finally:
        slot.close()
        plain.close()
        solid.close()


def test_frame_slot_lit_netc_with_self_shadow_in_a_lit_scene(ops, recon, nets):  # noqa: F811
    """shade="netC" over a lit scene with the self-shadow: the slot == render_mesh_many_in_scene with netC on the slot's
    own maps, and a frame whose mesh overflowed is coloured, lit, shadowed and composited again to the same bits."""
    from test_shadow_gpu import equal_pictures, slot_scene
    from test_slot_pictures_gpu import PICTURES as SLOT_PICTURES, SIZE, TWO, frames, make_slot
    images, calibs = frames()
    scene = slot_scene(recon)
    lighting = recon.Lighting(params(6)[0], direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), frame="camera", self_shadow=0.02)
    slot = make_slot(nets, {"normals": "accumulate", "colors": False}, dict(SLOT_PICTURES, shade="netC", scene=scene),
                     lighting=lighting)
    try:
        slot.submit(images, calibs, cameras=TWO)
        meshes, pics = slot.meshes(), slot.pictures()
        po = slot.picture_options
        nchw = slot.feats_hwc_c[0].permute(2, 0, 1)[None].contiguous()
        kw = dict(projection=po.projection, nearest=po.nearest, background=po.background, near=po.near,
                  perspective_correct=po.perspective_correct, composite="depth", netC=slot.netC,
                  feat_tensors_C=[[[nchw]], None], calib_tensors=[slot.calib[0:1], None])
        want = recon.render_mesh_many_in_scene(meshes, scene, TWO, SIZE, "netC", lighting=lighting, **kw)
        unlit = recon.render_mesh_many_in_scene(meshes, scene, TWO, SIZE, "netC", **kw)
        assert meshes[1] is None and equal_pictures(pics[0], want[0]) and equal_pictures(pics[1], want[1])
        changed = (pics[0].image != unlit[0].image).any(-1)
        assert changed.sum() > 60 and (pics[0].mask[changed] == 2).all() and equal_pictures(pics[1], unlit[1])
        assert (slot.light_shade[0] == 1.0).any() and (slot.light_shade[0] == 0.0).any()
        # the shade was made from the colour query's position picture before the paint: no position buffer of its own,
        # and the bits of the shade kernel on an explicit position pass
        assert not hasattr(slot, "light_pos")
        m, light = meshes[0], scene.light
        pos = ops.mesh_render_raw(m.verts.contiguous(), m.faces.contiguous(), mesh_counts(m), m.verts.contiguous(), TWO,
                                  SIZE, po.projection, po.nearest, background=po.background, near=po.near,
                                  perspective_correct=po.perspective_correct)
        shade = ops.picture_shadow_batch(None, [pos[0]], [pos[2]], [slot.shadow_depth[0]], [slot.shadow_face[0]],
                                         light.calib, light.projection, light.nearest, 0.02, light.radius,
                                         light.strength)[0][1]
        assert torch.equal(shade, slot.light_shade[0]) and torch.equal(pos[2], slot.light_face[0])
        first = [t.clone() for t in pics[0]]
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
            slot._render_pictures(2)
        slot._busy = True
        again = slot.pictures()
        assert slot._reran == [0] and int(again[1].mask.max()) == 1
        assert equal_pictures(again[0], first) and again[0].image.data_ptr() != slot.pictures_image[0].data_ptr()
    finally:
        slot.close()


def test_color_views_slot_with_lighting(recon, views_net, views_netc):
    """A multi-view slot takes ``lighting=`` through its constructor: == render_mesh(shade="netC", view=, lighting=) on
    its own mesh and maps; built with lighting=None it has none of the new buffers."""
    lighting = recon.Lighting(params(7)[0], direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), frame="camera")
    images, calibs = views_frames()
    cams = slot_cameras(2)
    mesh = {"normals": "accumulate", "colors": False}
    slot = colour_slot(views_net, views_netc, mesh=mesh, pictures=dict(NETC_PICTURES, background=BG), lighting=lighting)
    bare = colour_slot(views_net, views_netc, mesh=mesh, pictures=dict(NETC_PICTURES, background=BG), lighting=None)
    try:
        assert tuple(slot.light_normal.shape) == (2, 2, 40, 24, 3) and slot.lighting is lighting
        assert bare.lighting is None and not any(hasattr(bare, k) for k in LIGHT_BUFFERS)
        for s_ in (slot, bare):
            s_.submit(images, calibs, cameras=cams)
        meshes, pics, base = slot.meshes(), slot.pictures(), bare.pictures()
        assert meshes[1] is None and pics[1] is None and meshes[0].normals is not None
        nchw = torch.stack(own_maps(slot, 0)).permute(0, 3, 1, 2).contiguous()
        kw = dict(background=BG, netC=slot.netC, feat_tensor_C=[[nchw]], calib_tensor=slot.calib_in[0], view=slot.view)
        want = recon.render_mesh(meshes[0], cams[0], (40, 24), "netC", lighting=lighting, **kw)
        unlit = recon.render_mesh(meshes[0], cams[0], (40, 24), "netC", **kw)
        assert int((want.face >= 0).sum()) >= 100 and not torch.equal(want.image, unlit.image)
        for a, w, u in zip(pics[0], want, unlit):
            assert a.dtype == w.dtype and torch.equal(a.view(torch.int32), w.view(torch.int32))
        for a, u in zip(base[0], unlit):
            assert torch.equal(a.view(torch.int32), u.view(torch.int32))
    finally:
        slot.close()
        bare.close()
