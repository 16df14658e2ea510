"""pipeline.ColorViewsSlot on the GPU: a ViewsSlot with a multi-view netC.  The geometry is held to a ViewsSlot given the
same inputs, the textured render and the mesh colours to ops.query_views / recon.reconstruct_mesh(view=...) on the slot's
OWN netC maps and calibrations, bit for bit.  Needs an MI355X."""
import numpy as np
import pytest

import test_query_views_gpu as tv
from monoport_amd import synthetic as syn
from test_views_slot_gpu import HI, LO, RES, V, body_hook, frames, make_slot, net, same_mesh, vertices_equal  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
MESH = {"normals": "accumulate", "colors": True}


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops
    return ops


@pytest.fixture(scope="module")
def netc():
    """A multi-view netC of V views: the seeded head and encoder of the benchmark's netC."""
    n = tv._net("C", syn.rand_mlp("C", 61, 2.0), V)
    shapes = {k: tuple(v.shape) for k, v in n.image_filter.state_dict().items()}
    n.image_filter.load_state_dict({k: torch.from_numpy(v).to(DEV) for k, v in syn.seeded_state_dict(shapes, 72).items()})
    return n


def colour_slot(net, netc, **kw):
    from monoport_amd.pipeline import ColorViewsSlot
    kw.setdefault("mesh", MESH)
    return ColorViewsSlot(net, torch.device(DEV), netC=netc, batch=2, resolutions=RES, b_min=LO, b_max=HI,
                          feature_hook=body_hook(), **kw)


def own_maps(slot, f):
    return slot.feats_hwc_c[f * V:(f + 1) * V]


def want_render_tex(ops, slot, f):
    """paint of ops.query_views (what netC.query launches), row slot.view, on the slot's own netC maps and calib_in[f]
    over vertices[f]."""
    x, y, z, _, count = slot.vertices[f]
    c, r = int(count.item()), RES[-1]
    pts = ops.vertex_points(x, y, z, count, r, slot.mat_color)
    full = torch.zeros_like(pts)
    full[:, :c] = ops.query_views(slot.netC.surface_classifier.packed(), own_maps(slot, f),
                                  pts[:, :c][None].expand(V, 3, c), slot.calib_in[f], "orthogonal", syn.Z_SCALE)[slot.view]
    return c, ops.paint(x, y, full, 1, count, r, 0.5, 0.5, -np.inf, np.inf)


def want_mesh(slot, f):
    """recon.reconstruct_mesh(view=slot.view) on the slot's volume, own netC maps (back in NCHW) and calibrations."""
    from monoport_amd.recon import reconstruct_mesh
    nchw = torch.stack(own_maps(slot, f)).permute(0, 3, 1, 2).contiguous()
    return reconstruct_mesh(slot.volumes[f], 0.5, LO, HI, normals="accumulate", netC=slot.netC, feat_tensor_C=[[nchw]],
                            calib_tensor=slot.calib_in[f], view=slot.view)


def check_live_frame(ops, slot, f, what):
    c, tex = want_render_tex(ops, slot, f)
    # more than two tiles of the colour launch (G = 64 // V = 32 points each), so the tile loop and a partial tile run
    assert c > 64 and torch.equal(slot.renders_tex[f].view(torch.int32), tex.view(torch.int32)), what
    mesh = slot.meshes()[f]
    same_mesh(mesh, want_mesh(slot, f), what)
    assert mesh.colors.shape[0] > 64 and float(mesh.colors.min()) >= 0 and float(mesh.colors.max()) <= 1
    assert float(mesh.colors.std()) > 0.01
    return tex, mesh


def test_color_views_slot(ops, net, netc):
    from monoport_amd.pipeline import ColorViewsSlot, FramePipeline
    images, calibs = frames()
    slot = colour_slot(net, netc)
    plain = make_slot(net, mesh={"normals": "accumulate"})
    pipe = FramePipeline(net, torch.device(DEV), depth=1, batch=2, slot_class=ColorViewsSlot, netC=netc, resolutions=RES,
                         b_min=LO, b_max=HI, feature_hook=body_hook(), mesh=MESH)
    try:
        assert slot.views == V and len(slot.feats_hwc_c) == 2 * V and tuple(slot.image_c.shape) == (2 * V, 3, 512, 512)
        assert slot.mesh.colors and tuple(slot.image_c_in.shape) == (2, V, 3, 512, 512)
        slot.submit(images, calibs)
        plain.submit(images, calibs)
        slot.wait()
        plain.wait()
        # the geometry is the ViewsSlot's
        status = slot.status.tolist()
        print("ColorViewsSlot: status %s" % status)
        assert status == plain.status.tolist() and status[0][0] == 1 and status[1] == [0, 17 ** 3, 0, 0]
        assert torch.equal(slot.volumes[0], plain.volumes[0]) and vertices_equal(slot.vertices[0], plain.vertices[0])
        assert torch.equal(slot.renders[0], plain.renders[0])
        assert not torch.equal(own_maps(slot, 0)[0], own_maps(slot, 0)[1])  # netC's encoder saw batch * V images
        assert torch.equal(own_maps(slot, 0)[1][..., :256], slot.feats_hwc[1])  # feat_prior: netG's map of the image
        tex, mesh = check_live_frame(ops, slot, 0, "frame 0")
        meshes = slot.meshes()
        assert len(meshes) == 2 and meshes[1] is None
        same_mesh(mesh._replace(colors=None), plain.meshes()[0], "the ViewsSlot's mesh")
        first_tex, first_mesh = tex.clone(), type(mesh)(*[t.clone() for t in mesh])
        # FramePipeline with the slot class as a keyword: the same bits
        got = pipe.submit(images, calibs)
        got.wait()
        assert isinstance(got, ColorViewsSlot) and got.status.tolist() == status
        assert torch.equal(got.renders_tex[0].view(torch.int32), first_tex.view(torch.int32))
        same_mesh(got.meshes()[0], first_mesh, "FramePipeline")
        assert got.meshes()[1] is None
        # the frames swapped: the swapped results, nothing left over from the dead frame
        slot.submit(images.flip(0), calibs.flip(0))
        slot.wait()
        assert slot.status.tolist() == status[::-1]
        check_live_frame(ops, slot, 1, "swapped, frame 1")
        assert slot.meshes()[0] is None
        assert torch.equal(slot.renders_tex[1].view(torch.int32), first_tex.view(torch.int32))
        same_mesh(slot.meshes()[1], first_mesh, "swapped against the first submission")
    finally:
        slot.close()
        plain.close()
        pipe.close()


def test_view_row_selection(ops, net, netc):
    """Two live frames whose view-1 camera is shifted partly off its image: view = 1 holds the row under THAT view's
    mask, both in the volumes and in the colours, and differs from view = 0."""
    images, calibs = frames()
    images, calibs = images[[0, 0]].clone(), calibs[[0, 0]].clone()
    calibs[:, 1, 0, 3] += 0.7
    calibs[1, :, 0, 3] += 0.05
    slots = [colour_slot(net, netc, view=k) for k in range(V)]
    try:
        out = []
        for slot in slots:
            slot.submit(images, calibs)
            slot.wait()
            assert slot.status[:, 0].tolist() == [1, 1]
            out.append([check_live_frame(ops, slot, f, "view %d, frame %d" % (slot.view, f)) for f in range(2)])
        for f in range(2):
            assert not torch.equal(out[0][f][0], out[1][f][0])
            assert not torch.equal(slots[0].volumes[f], slots[1].volumes[f])
    finally:
        for slot in slots:
            slot.close()


def test_pictures_shade_colors(ops, net, netc):
    """pictures={"shade": "colors"} behind the multi-view colour chain: the image is the rasteriser's own call on the
    chain's buffers (netC's raw predictions, channel-major, painted as a * 0.5 + 0.5), as for FrameSlot."""
    images, calibs = frames()
    cam = torch.eye(4)[None]
    slot = colour_slot(net, netc, pictures={"views": 1, "res": 33, "shade": "colors"})
    try:
        slot.submit(images, calibs, cameras=cam)
        pics = slot.pictures()
        assert pics[1] is None and tuple(pics[0].image.shape) == (1, 33, 33, 3)
        buf = slot.mesh_buffers
        raw = ops.mesh_render_raw_batch([buf["verts"][0]], [buf["faces"][0]], [buf["counts"][0]], [buf["preds"][0]], [cam],
                                        33, "orthogonal", "max", channel_major=True, scale=0.5, bias=0.5, background=1.0)[0]
        hit = pics[0].face >= 0
        assert int(hit.sum()) > 60 and float(pics[0].image[hit].std()) > 0.01 and (pics[0].image[~hit] == 1.0).all()
        for a, b in zip(pics[0], raw):
            assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert (slot.pictures_image[1] == 1.0).all() and (slot.pictures_face[1] == -1).all()
        # the predictions the rasteriser read are the colour query's on the chain's own points
        nv = int(buf["counts"][0, 0].item())
        want = ops.query_views(slot.netC.surface_classifier.packed(), own_maps(slot, 0),
                               buf["points"][0][:, :nv][None].expand(V, 3, nv), slot.calib_in[0], "orthogonal",
                               syn.Z_SCALE)[slot.view]
        assert torch.equal(buf["preds"][0][:, :nv].view(torch.int32), want.view(torch.int32))
    finally:
        slot.close()
