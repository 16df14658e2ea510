"""tests/transfer_ref.py, the numpy restatement of mp_volume_bits / mp_mesh_transfer / mp_mesh_transfer_shade /
mp_picture_light_transfer (include/monoport_hip.h), held to np.packbits, to hand-made rays and -- independently of its
formulae -- to the float64 irradiance transfer A_l Y_lm(n) of an unoccluded sphere and to the half sky of a right-angle
corner; and the host logic of recon.Transfer, with_transfer, Lighting(transfer=) and the render calls.  No GPU."""
import inspect
import math

import numpy as np
import pytest

import light_ref
import transfer_ref as ref

F = np.float32

# (a) the sphere, D = 128, bias 1.5, step 1: max |prt - A_l Y_lm(n)| over the 16,206 marching-cubes vertices of
# sphere_volume(65, 0.9) with the analytic normal at each was 0.00733 (pure quadrature: analytic positions gave
# 0.0072); no ray with k > 0 was occluded.  (b) the corner at 33^3, the 14 floor vertices half a voxel and a voxel and a
# half from the wall along the middle of its length: max |prt_0 - 0.282095 pi / 2| was 0.0312 at D = 128 and 0.0388 at
# D = 512 -- quadrature (0.062 and 0.017 on the worst-placed vertex of an endless corner) and, with one sign at every
# D, the steep rays that leave through the top of the 33^3 box before they reach the wall.  The bounds are twice the
# measured values.
SPHERE_MEASURED = 0.00733
CORNER_MEASURED = {128: 0.0312, 512: 0.0388}


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- tables and bits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 512])
def test_tables_are_the_fibonacci_sphere_and_the_real_sh_basis(recon, d):
    t = recon.Transfer(directions=d)
    dirs, basis, weight = ref.tables(d)
    assert t.dirs.dtype == F and t.basis.dtype == F and t.dirs.shape == (d, 3) and t.basis.shape == (d, 9)
    assert np.array_equal(bits(t.dirs), bits(dirs)) and np.array_equal(bits(t.basis), bits(basis))
    assert t.weight == float(weight) == float(F(4 * math.pi / d))
    # what the tables are, not how they were made: unit vectors, evenly spaced in z, turning by the golden angle
    w = t.dirs.astype(np.float64)
    assert np.abs(np.linalg.norm(w, axis=1) - 1).max() < 1e-6
    assert np.allclose(w[:, 2], 1 - (2 * np.arange(d) + 1) / d, atol=1e-7)
    turn = np.diff(np.unwrap(np.arctan2(w[:, 1], w[:, 0])))
    assert np.allclose(np.mod(turn, 2 * math.pi), np.mod(math.pi * (3 - math.sqrt(5)), 2 * math.pi), atol=1e-4)
    # the basis is orthonormal under the quadrature (the order and constants of the lighting's H)
    gram = (t.basis.astype(np.float64).T @ t.basis.astype(np.float64)) * (4 * math.pi / d)
    assert np.abs(gram - np.eye(9)).max() < 3.0 / d
    x, y, z = w.T
    assert np.allclose(t.basis[:, 1] / t.basis[:, 3], y / x, rtol=1e-4)
    assert np.allclose(t.basis[:, 6], math.sqrt(5 / (16 * math.pi)) * (3 * z * z - 1), atol=1e-6)


@pytest.mark.parametrize("r", [1, 7, 17, 32, 33, 65])
def test_bits_are_packbits_of_the_comparison(r):
    rng = np.random.RandomState(r)
    vol = rng.uniform(0, 1, (r, r, r)).astype(F)
    flat = vol.reshape(-1)
    flat[rng.randint(0, flat.size, max(1, flat.size // 7))] = np.nan
    flat[rng.randint(0, flat.size, max(1, flat.size // 9))] = F(0.5)  # == level: empty
    flat[0] = np.inf
    got = ref.volume_bits(vol, 0.5)
    wx = (r + 31) // 32
    with np.errstate(invalid="ignore"):
        occ = vol > F(0.5)
    padded = np.zeros((r, r, wx * 32), bool)
    padded[:, :, :r] = occ
    want = np.packbits(padded, axis=-1, bitorder="little").view(np.uint32).reshape(-1)
    assert got.dtype == np.uint32 and got.shape == (r * r * wx,) == (ref.bits_words(r)[0],)
    assert np.array_equal(got, want)
    assert not occ[np.isnan(vol)].any() and not occ[vol == F(0.5)].any() and occ.reshape(-1)[0]
    if r % 32:  # the padding bits
        assert not (got.reshape(r, r, wx)[:, :, -1] >> np.uint32(r % 32)).any()
    assert np.array_equal(ref.occupancy(vol, 0.5), occ)


def test_bits_words(recon):
    from monoport_amd import ops
    for r, fine, blocks in ((1, 1, 1), (17, 17 * 17, 1), (33, 33 * 33 * 2, 4), (257, 257 * 257 * 9, 1124),
                            (513, 513 * 513 * 17, 8583)):
        assert ref.bits_words(r) == (fine, fine + blocks) and ops.volume_bits_words(r) == fine + blocks
    for bad in (0, 514, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            ops.volume_bits_words(bad)


# ---- hand-made rays ---------------------------------------------------------------------------------------------------
def trace(verts, normals, occ, dirs, bias_w=0.0, step_w=None, j=64, box=((-1, -1, -1), (1, 1, 1))):
    d = np.zeros((64, 3), F)
    d[:len(dirs)] = dirs
    basis = np.zeros((64, 9), F)
    basis[:, 0] = 1
    r = occ.shape[0]
    step_w = 2.0 / r if step_w is None else step_w
    return ref.transfer(np.asarray(verts, F), np.asarray(normals, F), occ, box[0], box[1], d, basis, 1.0, bias_w, step_w,
                        j)


def test_a_ray_is_traced_only_where_it_faces_away_and_stops_at_the_first_set_voxel():
    occ = np.zeros((8, 8, 8), bool)
    occ[6, 3, 3] = True  # z = 6, y = 3, x = 3
    centre = [(3.5 / 8) * 2 - 1] * 3  # the middle of voxel (3, 3, 3)
    up, down, side = (0, 0, 1), (0, 0, -1), (1, 0, 0)
    mask, prt, samples = trace([centre], [up], occ, [up, down, side, (0, 1, 0), (0, 0.6, 0.8)])
    # up: k = 1, hits z = 6 at j = 3: occluded.  down: k < 0.  side, (0,1,0): k = 0, not > 0.  tilted: k = 0.8, passes
    assert mask[0, 0] == 1 << 4 and samples == 4 + 7
    assert np.array_equal(prt[0], np.array([F(0.8)] + [0] * 8, F))
    # the blocker one voxel aside: the ray leaves through the top, bit 1
    mask, _, _ = trace([centre], [up], np.roll(occ, 1, 2), [up])
    assert mask[0, 0] == 1
    # a reach that stops in front of the blocker: unoccluded
    assert trace([centre], [up], occ, [up], j=3)[0][0, 0] == 1 and trace([centre], [up], occ, [up], j=4)[0][0, 0] == 0
    # bias 0 in a set voxel: the ray hits itself at j = 0; a bias of a voxel and a half lifts it out
    own = np.zeros((8, 8, 8), bool)
    own[3, 3, 3] = True
    assert trace([centre], [up], own, [up])[0][0, 0] == 0
    assert trace([centre], [up], own, [up], bias_w=1.5 * 2 / 8)[0][0, 0] == 1
    # a vertex outside the box: every ray that is traced has left at j = 0
    mask, _, samples = trace([[0, 0, 1.5]], [up], np.ones((8, 8, 8), bool), [up, (0, 0.6, 0.8), down])
    assert mask[0, 0] == 0b011 and samples == 2
    # zero, NaN and inf normals: u = 0, k = 0, nothing is traced, prt = 0
    for n in ([0, 0, 0], [np.nan, 0, 1], [0, np.inf, 0]):
        mask, prt, samples = trace([centre], [n], occ, [up, down, side])
        assert mask[0, 0] == 0 and samples == 0 and not prt.any()


def test_the_sum_runs_over_the_seen_directions_in_ascending_order():
    rng = np.random.RandomState(3)
    dirs, basis, weight = ref.tables(64)
    basis = (basis * rng.uniform(0.5, 2, basis.shape)).astype(F)
    occ = np.zeros((4, 4, 4), bool)
    n = np.array([[0.3, -0.5, 0.8]], F)
    mask, prt, _ = ref.transfer(np.zeros((1, 3), F), n, occ, (-1,) * 3, (1,) * 3, dirs, basis, weight, 0.0, 0.5, 16)
    u = light_ref.normalise(n)[0]
    acc = np.zeros(9, F)
    want_mask = 0
    for d in range(64):
        k = (dirs[d, 0] * u[0] + dirs[d, 1] * u[1]) + dirs[d, 2] * u[2]
        if k > 0:
            want_mask |= 1 << d
            acc = acc + (k * basis[d])
    assert int(mask[0, 0]) == want_mask and np.array_equal(bits(prt[0]), bits(acc * weight))
    back = np.zeros(9, F)
    for d in reversed(range(64)):
        k = (dirs[d, 0] * u[0] + dirs[d, 1] * u[1]) + dirs[d, 2] * u[2]
        if k > 0:
            back = back + (k * basis[d])
    assert not np.array_equal(bits(back * weight), bits(prt[0]))  # the order matters to the bits


def test_shade_and_light_transfer():
    rng = np.random.RandomState(5)
    prt = rng.standard_normal((7, 9)).astype(F)
    sh = rng.uniform(-0.6, 0.9, (9, 3)).astype(F)
    t = ref.shade(prt, sh)
    want = np.zeros((7, 3), F)
    for k in range(9):
        want = want + prt[:, k, None] * sh[k][None, :]
    assert np.array_equal(bits(t), bits(want))
    # the lighting with the ambient picture: light_ref.light's steps around a replaced step 4
    normal = rng.standard_normal((12, 3)).astype(F)
    face = np.array([0, 1, -1, 2, 3, 4, -1, 5, 6, 7, 8, 9], np.int32)
    albedo = rng.uniform(0, 1, (12, 3)).astype(F)
    amb = rng.uniform(-0.2, 1.5, (12, 3)).astype(F)
    image, shading = ref.light_transfer(amb, None, face, albedo)
    cov = face >= 0
    assert np.array_equal(bits(shading[cov]), bits(amb[cov])) and not shading[~cov].any()
    assert np.array_equal(bits(image[~cov]), bits(albedo[~cov]))
    assert np.array_equal(bits(image[cov]), bits(np.clip(albedo[cov] * amb[cov], 0, 1)))
    # an SH lighting of coefficient 0 alone is an ambient of H0 * sh0: both entry points then agree on the bits
    sh0 = np.zeros((9, 3), F)
    sh0[0] = (0.7, 0.8, 0.9)
    const = np.broadcast_to(F(light_ref.C4) * sh0[0], (12, 3))
    kw = dict(direct_dir=(0, -0.6, 0.8), direct_rgb=(1, 0.5, 0.25), visibility=rng.uniform(0, 1, 12).astype(F))
    for gamma in (1.0, 2.2):
        a = ref.light_transfer(const, normal, face, albedo, gamma=gamma, **kw)
        b = light_ref.light(normal, face, albedo, sh0, gamma=gamma, **kw)
        # H_i * 0 adds +0.0 eight times: the same bits unless a sum is -0.0, which c4 * sh0 > 0 excludes
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
    image, _ = ref.light_transfer(amb, None, face, None, albedo_rgb=(0.5, 0.5, 0.5), background=0.25)
    assert (image[~cov] == F(0.25)).all()


# ---- two tests that do not lean on the restatement's formulae ---------------------------------------------------------
def irradiance_transfer(n):
    """float64 A_l Y_lm(n), written out: the transfer of an unoccluded surface with normal n [N,3]."""
    x, y, z = n[:, 0], n[:, 1], n[:, 2]
    pi = math.pi
    a0, a1, a2 = pi, 2 * pi / 3, pi / 4
    return np.stack([a0 * 0.28209479177387814 * np.ones_like(x),
                     a1 * 0.4886025119029199 * y, a1 * 0.4886025119029199 * z, a1 * 0.4886025119029199 * x,
                     a2 * 1.0925484305920792 * x * y, a2 * 1.0925484305920792 * y * z,
                     a2 * 0.31539156525252005 * (3 * z * z - 1), a2 * 1.0925484305920792 * z * x,
                     a2 * 0.5462742152960396 * (x * x - y * y)], 1)


def test_unoccluded_transfer_is_the_irradiance_transfer_of_the_normal():
    from monoport_amd import synthetic
    from oracle import pifu_oracle
    vol = synthetic.sphere_volume(65, 0.9)
    verts, _ = pifu_oracle.marching_cubes(vol)
    verts = np.ascontiguousarray(verts, F)
    n64 = verts.astype(np.float64)
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    normals = n64.astype(F)
    dirs, basis, weight = ref.tables(128)
    bias_w, step_w, steps = ref.rays(65, (-1,) * 3, (1,) * 3)
    mask, prt, _ = ref.transfer(verts, normals, ref.occupancy(vol, 0.5), (-1,) * 3, (1,) * 3, dirs, basis, weight,
                                bias_w, step_w, steps)
    facing = (normals.astype(np.float64) @ dirs.astype(np.float64).T) > 1e-6
    seen = ((mask[:, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    seen = seen.reshape(verts.shape[0], -1)
    assert verts.shape[0] > 10000 and not (facing & ~seen).any()  # a convex body occludes none of its own rays
    err = float(np.abs(prt.astype(np.float64) - irradiance_transfer(n64)).max())
    print("sphere65: max |prt - A_l Y_lm(n)| = %.5f over %d vertices" % (err, verts.shape[0]))
    assert err <= 2 * SPHERE_MEASURED


@pytest.mark.parametrize("d", [128, 512])
def test_a_right_angle_corner_sees_half_the_sky(d):
    from oracle import pifu_oracle
    r, thick = 33, 4
    vol = ref.corner(r, thick)
    verts, _ = pifu_oracle.marching_cubes(vol)
    g = (verts.astype(np.float64) + 1) / 2 * r  # (x, y, z) in voxels
    # the floor's top, within two voxels of the wall, in the middle of the wall's length (near its ends a ray leaves
    # the box sideways before it reaches the wall)
    middle = (np.abs(g[:, 2] - thick) < 1e-3) & (np.abs(g[:, 1] - r / 2) <= 4)
    floor = middle & (g[:, 0] > thick) & (g[:, 0] <= thick + 2)
    far = middle & (g[:, 0] >= r - 12) & (g[:, 0] <= r - 10)  # the same floor, far from the wall
    assert floor.sum() >= 12 and far.sum() >= 12
    dirs, basis, weight = ref.tables(d)
    bias_w, step_w, steps = ref.rays(r, (-1,) * 3, (1,) * 3)
    up = np.broadcast_to(np.array([0, 0, 1], F), verts.shape)
    _, prt, _ = ref.transfer(verts[floor | far], up[floor | far], ref.occupancy(vol, 0.5), (-1,) * 3, (1,) * 3, dirs,
                             basis, weight, bias_w, step_w, steps)
    near = prt[floor[floor | far]][:, 0].astype(np.float64)
    open_sky = prt[far[floor | far]][:, 0].astype(np.float64)
    err = float(np.abs(near - 0.282095 * math.pi / 2).max())
    print("corner33 D=%d: max |prt_0 - Y_00 pi / 2| = %.4f over %d vertices" % (d, err, near.size))
    assert err <= 2 * CORNER_MEASURED[d]
    # the open floor, 18 to 20 voxels from the 29-voxel wall, sees all of the sky but what lies below 58 degrees in the
    # half towards the wall: at most cos^2(58 deg) = 0.28 of that half's cosine-weighted share
    full = 0.282095 * math.pi
    print("           open floor: prt_0 in %.4f .. %.4f of %.4f" % (open_sky.min(), open_sky.max(), full))
    assert (open_sky >= full * (1 - 0.5 * 0.28) - 2 * CORNER_MEASURED[d]).all()
    assert (open_sky <= full + 2 * CORNER_MEASURED[d]).all() and open_sky.min() > near.max() + 0.2


# ---- the Python surface -----------------------------------------------------------------------------------------------
def test_transfer_validates_in_the_constructor(recon):
    t = recon.Transfer()
    assert (t.directions, t.bias, t.step, t.reach) == (128, 1.5, 1.0, None)
    assert recon.Transfer(64, 0, 0.5, 10).rays(33, (-1,) * 3, (1,) * 3) == (0.0, float(F(0.5 * 2 / 33)), 20)
    # voxels are measured on the smallest edge; the default reach crosses the box's diagonal
    bias_w, step_w, steps = t.rays(33, (-1, -2, -1), (1, 2, 3))
    assert (bias_w, step_w, steps) == tuple(float(v) if i < 2 else v for i, v in enumerate(
        ref.rays(33, (-1, -2, -1), (1, 2, 3)))) and steps == math.ceil(math.sqrt(3) * 33) + 2
    assert step_w == float(F(2 / 33))
    for bad in (dict(directions=0), dict(directions=100), dict(directions=576), dict(directions=128.0),
                dict(directions=True), dict(directions="128"), dict(bias=-0.5), dict(bias=np.nan), dict(bias="1"),
                dict(bias=None), dict(step=0), dict(step=-1), dict(step=np.inf), dict(step=None), dict(reach=0),
                dict(reach=-3), dict(reach=np.nan), dict(reach="far"), dict(reach=True)):
        with pytest.raises(ValueError):
            recon.Transfer(**bad)


def test_lighting_with_transfer_and_the_render_calls_refuse_before_anything_is_enqueued(recon):
    import torch
    sh = np.random.RandomState(0).uniform(-0.6, 0.9, (9, 3)).astype(F)
    t = recon.Transfer(64)
    lit = recon.Lighting(sh, transfer=t)
    assert lit.transfer is t and recon.Lighting(sh).transfer is None
    assert list(inspect.signature(recon.Lighting.__init__).parameters)[-1] == "transfer"
    assert inspect.signature(recon.Lighting.__init__).parameters["transfer"].default is None
    for bad in ("prt", 128, {"directions": 128}):
        with pytest.raises(ValueError, match="Transfer"):
            recon.Lighting(sh, transfer=bad)
    with pytest.raises(ValueError, match="camera"):
        recon.Lighting(sh, frame="camera", transfer=t)
    verts, faces = torch.zeros(3, 3), torch.zeros((1, 3), dtype=torch.int32)
    mesh = recon.Mesh(verts, faces, torch.zeros(3, 3), torch.zeros(3, 3))
    cam = np.eye(4, dtype=F)
    scene = object.__new__(recon.Scene)
    scene.light = None
    for call in (recon.render_mesh, lambda m, *a, **k: recon.render_mesh_many([m], *a, **k),
                 lambda m, *a, **k: recon.render_mesh_many_in_scene([m], scene, *a, **k)):
        with pytest.raises(ValueError, match="with_transfer"):
            call(mesh, cam, 8, "colors", lighting=lit)
        with pytest.raises(ValueError, match="with_transfer"):  # a transfer of another mesh
            call(_resized(recon, mesh), cam, 8, "colors", lighting=lit)
        sneaked = recon.Lighting(sh, transfer=t)
        sneaked.frame = "camera"
        with pytest.raises(ValueError, match="camera"):
            call(recon.with_transfer(mesh, torch.zeros(3, 9)), cam, 8, "colors", lighting=sneaked)
    assert recon.render_mesh(None, cam, 8, "colors", lighting=lit) is None
    # with_transfer: a Mesh of the same four fields that carries .transfer
    prt = torch.zeros(3, 9)
    carried = recon.with_transfer(mesh, prt)
    assert isinstance(carried, recon.Mesh) and carried._fields == recon.Mesh._fields and carried.transfer is prt
    assert tuple(carried) == tuple(mesh) and len(carried) == 4 and carried.verts is mesh.verts
    assert recon.Mesh(*[f for f in carried]) == mesh and not hasattr(mesh, "transfer")
    assert recon.with_transfer(None, prt) is None
    for bad in (torch.zeros(4, 9), torch.zeros(3, 3), torch.zeros(27), None, np.zeros((3, 9), F)):
        with pytest.raises(ValueError, match="prt"):
            recon.with_transfer(mesh, bad)
    # mesh_transfer
    vol = torch.zeros(8, 8, 8)
    with pytest.raises(ValueError, match="Transfer"):
        recon.mesh_transfer(mesh, vol, "transfer")
    with pytest.raises(ValueError, match="normals"):
        recon.mesh_transfer(mesh._replace(normals=None), vol, t)
    with pytest.raises(ValueError, match="cubic"):
        recon.mesh_transfer(mesh, torch.zeros(8, 8, 4), t)
    with pytest.raises(ValueError, match="resolution"):
        recon.mesh_transfer(mesh, torch.zeros(1, 1, 1).expand(514, 514, 514), t)


def _resized(recon, mesh):
    import torch
    out = recon.with_transfer(mesh, torch.zeros(3, 9))
    out.transfer = torch.zeros(4, 9)
    return out


def test_the_raw_wrappers_refuse_bad_host_values():
    import torch
    from monoport_amd import ops
    dirs, basis = torch.zeros(64, 3), torch.zeros(64, 9)
    good = dict(r=33, b_min=(-1,) * 3, b_max=(1,) * 3, n_dirs=64, dirs=dirs, basis=basis, weight=0.1, bias_w=0.1,
                step_w=0.06, max_steps=60)
    ops.transfer_params("t", **good)
    for bad in (dict(r=0), dict(r=514), dict(r=33.0), dict(n_dirs=32), dict(n_dirs=96), dict(n_dirs=576),
                dict(max_steps=0), dict(max_steps=(1 << 24) + 1), dict(max_steps=2.5), dict(b_min=(1, -1, -1)),
                dict(b_max=(1, 1, np.nan)), dict(b_min=(-1, -1)), dict(weight=np.inf), dict(bias_w=np.nan),
                dict(step_w=0), dict(step_w=-0.1), dict(dirs=torch.zeros(64, 4)), dict(basis=torch.zeros(64, 3)),
                dict(dirs=np.zeros((64, 3), F)), dict(basis=torch.zeros(64, 9, dtype=torch.float64)),
                dict(dirs=torch.zeros(128, 3)[::2])):
        with pytest.raises(ValueError):
            ops.transfer_params("t", **dict(good, **bad))


def test_the_pins_hold(recon):
    from monoport_amd import pipeline
    assert recon.Mesh._fields == ("verts", "faces", "normals", "colors")
    assert recon.MeshOptions._fields == ("normals", "level", "colors", "clean", "simplify", "smooth")
    assert pipeline.PICTURE_KEYS == ("views", "res", "shade", "projection", "nearest", "near", "perspective_correct",
                                     "background", "scene", "composite")
    assert pipeline.PictureOptions._fields == pipeline.PICTURE_KEYS
    for fn in (recon.render_mesh, recon.render_mesh_many, recon.render_mesh_many_in_scene, pipeline.FrameSlot.__init__):
        last = list(inspect.signature(fn).parameters.items())[-1]
        assert last[0] == "lighting" and last[1].default is None
    assert list(inspect.signature(recon.Lighting.__init__).parameters)[1:7] == ["sh", "direct", "gamma", "frame",
                                                                               "albedo", "self_shadow"]
    assert list(inspect.signature(recon.Transfer.__init__).parameters)[1:] == ["directions", "bias", "step", "reach"]
    assert [inspect.signature(recon.Transfer.__init__).parameters[k].default
            for k in ("directions", "bias", "step", "reach")] == [128, 1.5, 1.0, None]
