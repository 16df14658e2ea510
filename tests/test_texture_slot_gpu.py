"""netC baked into the atlas, on the GPU: recon.bake_texture's covered texels equal netC's own query (ops.query; for a
multi-view head ops.query_views) on the point list that the numpy restatements make of the atlas, bit for bit, and the
rest is the background; FrameSlot / ColorViewsSlot.encode_meshes(Glb(texture=Atlas(...))) lay out behind their mesh
chain the files that recon.encode_glb makes of slot.meshes(), byte for byte, through a capacity too small and an image
capacity too small as well; an atlas too small raises; slots without netC refuse.  Needs an MI355X."""
import numpy as np
import pytest

import atlas_ref
import glb_ref
import glb_texture_ref as tex
import picture_ref
import test_query_views_gpu as tv
from monoport_amd import synthetic as syn
from test_color_views_slot_gpu import netc as views_netc, own_maps  # noqa: F401  (netc: the fixture)
from test_mesh_batch_gpu import BMAX, BMIN, _body_hook, nets  # noqa: F401  (nets: the fixture)
from test_render_netc_gpu import RES, bits, count_colour_queries, heads, mesh33, slot_frames  # noqa: F401  (fixtures)
from test_views_slot_gpu import HI, LO, V, body_hook, frames as views_frames, make_slot as make_views_slot, net as views_net  # noqa: F401,E501

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BACKGROUND = 0.25
MESH = {"simplify": 16, "normals": "accumulate", "colors": False}


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def want_texture(mesh, atlas, query):
    """The definition: the restated atlas of the mesh, the restated list of its covered texels, ``query`` (points
    [3,n] on the device -> predictions [3,n]) on that list, the restated paint.  -> (image, face_id, covered)."""
    face, pos, info = atlas_ref.atlas(mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), atlas.size, atlas.cell,
                                      atlas.background)
    assert info[0] == info[1] == mesh.faces.shape[0]
    pts, pix, count = picture_ref.points(face, pos)
    n = int(count[0])
    preds = np.zeros_like(pts)
    preds[:, :n] = query(torch.from_numpy(pts[:, :n].copy()).to(DEV)).cpu().numpy()
    return picture_ref.paint(preds, pix, count, pos.copy()), face, n


@pytest.mark.parametrize("calibration,maps,size,cell", [("orthogonal", "48x80", 512, 4), ("perspective", "64x64", 512, 7),
                                                        ("orthogonal", "64x64", 1024, 13)])
def test_bake_texture_is_the_query(ops, recon, mesh33, heads, calibration, maps, size, cell):  # noqa: F811
    net, calib, feat = heads["nets"][calibration], heads["calibs"][calibration], heads["maps"][maps]
    atlas = recon.Atlas(size, cell, background=BACKGROUND)
    image, face = recon.bake_texture(mesh33, atlas, netC=net, feat_tensors_C=feat, calib_tensors=calib)
    b = recon._bind_netC("test", net, [(feat, calib, torch.device(DEV))])[0]
    want, want_face, covered = want_texture(
        mesh33, atlas, lambda pts: ops.query(b.mlp, b.feat_hwc, pts[None], b.calib, b.z_scale, b.projection)[0])
    print("%s / %s / Atlas(%d, %d): %d faces, %d of %d texels queried"
          % (calibration, maps, size, cell, mesh33.faces.shape[0], covered, size * size))
    assert covered >= 1000 and tuple(image.shape) == (size, size, 3)
    assert np.array_equal(face.cpu().numpy(), want_face)
    assert np.array_equal(bits(image), bits(want))
    off = face < 0
    assert bool((image[off] == BACKGROUND).all()) and float(image[~off].std()) > 0.01
    # a list of one mesh is the single call, and two meshes of different sizes each equal theirs
    other = recon.Mesh(mesh33.verts[:900].contiguous(), mesh33.faces[(mesh33.faces < 900).all(1)].contiguous(), None, None)
    images, faces = recon.bake_texture([mesh33, other], atlas, netC=net, feat_tensors_C=[feat, feat],
                                       calib_tensors=[calib, calib])
    alone = recon.bake_texture(other, atlas, netC=net, feat_tensors_C=feat, calib_tensors=calib)
    assert np.array_equal(bits(images[0]), bits(image)) and np.array_equal(bits(images[1]), bits(alone[0]))
    assert torch.equal(faces[1], alone[1]) and not torch.equal(faces[0], faces[1])


def test_bake_texture_multi_view_head(ops, recon, mesh33):  # noqa: F811
    """view=k of a V = 2 head: row k of ops.query_views on the same points."""
    net2 = tv._net("C", syn.rand_mlp("C", 61, 2.0), V)
    feat = [[torch.from_numpy(np.stack([syn.rand_feat(512, 48, 80, 70 + v) for v in range(V)])).to(DEV)]]
    calibs = torch.stack([torch.eye(4) * 0.9, torch.eye(4)]).to(DEV)
    calibs[1, 0, 3] = -0.7
    atlas = recon.Atlas(512, 5, background=BACKGROUND)
    images = []
    for k in range(V):
        image, face = recon.bake_texture(mesh33, atlas, netC=net2, feat_tensors_C=feat, calib_tensors=calibs, view=k)
        b = recon._bind_netC("test", net2, [(feat, calibs, torch.device(DEV))], view=k)[0]

        def query(pts, k=k, b=b):
            return ops.query_views(b.mlp, b.maps, pts[None].expand(V, 3, pts.shape[1]), b.calibs, b.projection, b.z_scale)[k]

        want, want_face, covered = want_texture(mesh33, atlas, query)
        assert covered >= 1000 and np.array_equal(face.cpu().numpy(), want_face)
        assert np.array_equal(bits(image), bits(want)), k
        images.append(image)
    assert not torch.equal(images[0], images[1])
    with pytest.raises(NotImplementedError, match="view="):
        recon.bake_texture(mesh33, atlas, netC=net2, feat_tensors_C=feat, calib_tensors=calibs)
    with pytest.raises(ValueError, match="one of the two"):
        recon.bake_texture(mesh33, atlas)
    with pytest.raises(ValueError, match="recon.Atlas"):
        recon.bake_texture(mesh33, (512, 5), colors=lambda p: p)


# ---- the slots --------------------------------------------------------------------------------------------------------
ATLAS = (128, 8)


def check_glbs(recon, slot, glb, live, maps_of, calib_of, view=None):
    """slot.glbs() against recon.encode_glb of slot.meshes() on the slot's own maps and calibrations."""
    files, meshes = slot.glbs(), slot.meshes()
    assert len(files) == len(meshes) == slot.n_active == len(live)
    for b, (f, mesh) in enumerate(zip(files, meshes)):
        if not live[b]:
            assert f is None and mesh is None
            continue
        nf = mesh.faces.shape[0]
        assert isinstance(f, bytes) and 30 < nf <= glb.texture.faces and mesh.colors is None
        want = recon.encode_glb(mesh, glb, BMIN, BMAX, netC=slot.netC, feat_tensors_C=[[maps_of(b)]],
                                calib_tensors=calib_of(b), view=view)
        assert f == want, b
        got = tex.read(f)
        assert len(got["positions"]) == 3 * nf and len(f) == tex.file_bytes(nf, len(got["png"]), glb.normals)
        corner = mesh.faces.cpu().numpy().reshape(-1)
        assert np.abs(got["positions"] - mesh.verts.cpu().numpy().astype(np.float64)[corner]).max() <= 0.52 * 2.0 / 65535
        image = tex.decode_png(got["png"])
        assert image.shape == (glb.texture.size, glb.texture.size, 3) and len(np.unique(image)) > 10  # netC did arrive
    return files


def frame_maps(slot):
    return (lambda b: slot.feats_hwc_c[b].permute(2, 0, 1)[None].contiguous()), (lambda b: slot.calib[b:b + 1])


def make_frame_slot(nets, netc=True, mesh=MESH):  # noqa: F811
    from monoport_amd.pipeline import FrameSlot
    return FrameSlot(nets[0], torch.device(DEV), netC=nets[1] if netc else None, batch=3, resolutions=RES, b_min=BMIN,
                     b_max=BMAX, feature_hook=_body_hook(), mesh=mesh)


def test_frame_slot(ops, recon, nets, monkeypatch):  # noqa: F811
    images, calibs = slot_frames()
    glb = recon.Glb(texture=recon.Atlas(*ATLAS))
    slot, plain = make_frame_slot(nets), make_frame_slot(nets)
    try:
        new = ("atlas_face", "atlas_image", "atlas_info", "atlas_lists", "atlas_png", "atlas_png_info")
        assert not any(hasattr(slot, k) for k in new)
        slot.encode_meshes(glb)
        plain.encode_meshes(recon.Glb(colors=False))
        assert not any(hasattr(plain, k) for k in new)  # a plain Glb: nothing of the texture's
        a = ATLAS[0]
        assert tuple(slot.atlas_face.shape) == (3, a, a) and tuple(slot.atlas_image.shape) == (3, a, a, 3)
        assert {k: tuple(v.shape) for k, v in slot.atlas_lists.items()} == {
            "points": (3, 3, a * a), "pixels": (3, a * a), "preds": (3, 3, a * a), "count": (3, 2)}
        assert sum(v[0].numel() * v.element_size() for v in slot.atlas_lists.values()) == 28 * a * a + 8
        assert tuple(slot.atlas_png.shape) == (3, glb.texture.png_capacity()) and tuple(slot.atlas_png_info.shape) == (3, 2)
        cap_v = 12 * RES[-1] ** 2
        assert tuple(slot.glb_bytes.shape) == (3, glb.capacity_for(cap_v, 2 * cap_v))
        assert not slot.mesh.colors and "preds" not in slot.mesh_buffers
        calls = count_colour_queries(ops, monkeypatch)
        slot.submit(images, calibs)
        slot.wait()
        monkeypatch.undo()
        plain.submit(images, calibs)
        plain.wait()
        assert slot.status[:, 0].tolist() == [1, 0, 1]
        # the colour queries of the submission: the textured render's over the r^2 columns and the atlas's over its
        # texels -- none over the mesh's vertex capacity
        assert sorted(set(calls)) == [("query_counted_batch", 33 * 33), ("query_counted_batch", a * a)], calls
        files = check_glbs(recon, slot, glb, (True, False, True), *frame_maps(slot))
        assert files[0] != files[2]
        info = slot.glb_info.cpu().numpy()
        assert [tuple(r) for r in info] == [(len(files[0]), 0), (glb_ref.MIN_BYTES, 0), (len(files[2]), 0)]
        atlas_info = slot.atlas_info.cpu().tolist()
        assert atlas_info[1] == [0, 0] and atlas_info[0][0] == atlas_info[0][1] == slot.meshes()[0].faces.shape[0]
        assert bool((slot.atlas_face[1] == -1).all()) and bool((slot.atlas_image[1] == 0.5).all())
        assert torch.equal(plain.meshes()[0].verts, slot.meshes()[0].verts)  # the chain is untouched
        # the slot's own buffers hold the bake of its meshes
        image, face = recon.bake_texture(slot.meshes()[0], glb.texture, netC=slot.netC,
                                         feat_tensors_C=[[frame_maps(slot)[0](0)]], calib_tensors=slot.calib[0:1])
        assert torch.equal(face, slot.atlas_face[0]) and np.array_equal(bits(image), bits(slot.atlas_image[0]))
        covered = int((face >= 0).sum())
        assert slot.atlas_lists["count"].tolist()[0] == [covered, covered]
        print("FrameSlot frame 0: %d faces, %d of %d texels queried, %d bytes" % (atlas_info[0][1], covered, a * a, len(files[0])))
        # a short batch behind it
        slot.submit(images[:1], calibs[:1])
        assert check_glbs(recon, slot, glb, (True,), *frame_maps(slot))[0] == files[0]
    finally:
        slot.close()
        plain.close()


def test_short_capacities_and_an_atlas_too_small(recon, nets):  # noqa: F811
    images, calibs = slot_frames()
    roomy = recon.Glb(texture=recon.Atlas(*ATLAS))
    slots = [make_frame_slot(nets) for _ in range(4)]
    try:
        slots[0].encode_meshes(roomy)
        slots[0].submit(images, calibs)
        files = slots[0].glbs()
        assert files[1] is None and len(files[0]) > 4096
        # the file's capacity forced short: code 1, the size reported, the same bytes from glbs()
        slots[1].encode_meshes(recon.Glb(texture=recon.Atlas(*ATLAS), capacity=len(files[0]) // 2))
        slots[1].submit(images, calibs)
        slots[1].wait()
        info = slots[1].glb_info.cpu().numpy()
        assert tuple(info[0]) == (len(files[0]), 1) and tuple(info[1]) == (glb_ref.MIN_BYTES, 0)
        assert slots[1].glbs() == files
        # the image's capacity forced short: code 2 with room in the atlas -- baked and encoded again, the same bytes
        slots[2].encode_meshes(recon.Glb(texture=recon.Atlas(*ATLAS, png_capacity=100)))
        slots[2].submit(images, calibs)
        slots[2].wait()
        info = slots[2].glb_info.cpu().numpy()
        assert [tuple(r) for r in info] == [(0, 2), (glb_ref.MIN_BYTES, 0), (0, 2)]
        assert slots[2].atlas_png_info[0, 1].item() == 1
        assert slots[2].glbs() == files
        # an atlas that is too small: the device says so, glbs() raises with both numbers
        slots[3].encode_meshes(recon.Glb(texture=recon.Atlas(64, 32)))
        slots[3].submit(images, calibs)
        slots[3].wait()
        assert slots[3].glb_info.cpu().numpy()[0].tolist() == [0, 2]
        nf = slots[3].meshes()[0].faces.shape[0]
        assert slots[3].atlas_info.cpu().tolist()[0] == [8, nf]
        with pytest.raises(ValueError, match="%d faces and Atlas\\(64, 32\\) holds 8" % nf):
            slots[3].glbs()
        # the mesh capacity cut behind the good submission: glbs() encodes the re-run mesh
        slot = slots[0]
        for k, v in slot.mesh_buffers.items():
            cut = {"verts": 100, "normals": 100, "simple_verts": 100, "simple_vmap": 100, "faces": 200, "simple_faces": 200}
            slot.mesh_buffers[k] = v[:, :cut[k]] if k in cut else v
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(3)
        slot._busy = True
        again = slot.glbs()
        assert 0 in slot._reran and again == files
    finally:
        for s in slots:
            s.close()


def test_color_views_slot(ops, recon, views_net, views_netc, monkeypatch):  # noqa: F811
    from monoport_amd.pipeline import ColorViewsSlot
    images, calibs = views_frames()
    images, calibs = torch.cat([images, images[:1]]), torch.cat([calibs, calibs[:1]])
    glb = recon.Glb(texture=recon.Atlas(*ATLAS))
    slot = ColorViewsSlot(views_net, torch.device(DEV), netC=views_netc, batch=3, resolutions=list(RES), b_min=LO, b_max=HI,
                          feature_hook=body_hook(), mesh=MESH)
    try:
        slot.encode_meshes(glb)
        calls = count_colour_queries(ops, monkeypatch)
        slot.submit(images, calibs)
        slot.wait()
        monkeypatch.undo()
        assert slot.status[:, 0].tolist() == [1, 0, 1]
        a = ATLAS[0]
        assert sorted(set(calls)) == [("query_views_counted_batch", 33 * 33), ("query_views_counted_batch", a * a)], calls
        files = check_glbs(recon, slot, glb, (True, False, True),
                           lambda b: torch.stack(list(own_maps(slot, b))).permute(0, 3, 1, 2).contiguous(),
                           lambda b: slot.calib_in[b], view=slot.view)
        assert files[0] == files[2]  # the same frame twice
    finally:
        slot.close()


def test_what_a_slot_refuses(recon, nets, views_net):  # noqa: F811
    from monoport_amd.pipeline import FramePipeline
    textured = recon.Glb(normals=False, texture=recon.Atlas(*ATLAS))
    bare = make_frame_slot(nets, netc=False, mesh={"normals": None, "colors": False})
    views = make_views_slot(views_net, mesh={"normals": None})
    try:
        for slot in (bare, views):
            with pytest.raises(ValueError, match="netC"):
                slot.encode_meshes(textured)
            assert slot.glb is None and not hasattr(slot, "glb_bytes") and not hasattr(slot, "atlas_face")
    finally:
        bare.close()
        views.close()
    pipe = FramePipeline(nets[0], torch.device(DEV), depth=1, batch=1, netC=nets[1], resolutions=RES, b_min=BMIN, b_max=BMAX,
                         mesh={"normals": None, "colors": False})
    try:
        pipe.encode_meshes(textured)
        assert pipe.slots[0].glb is textured and tuple(pipe.slots[0].atlas_face.shape) == (1, 128, 128)
    finally:
        pipe.close()
