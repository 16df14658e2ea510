"""FrameSlot.encode_meshes(recon.Glb) / glbs and recon.encode_glb on the GPU: the files a slot lays out behind each chunk
of its mesh chain, on its own stream and from the chain's own buffers and device counts, equal recon.encode_glb of
slot.meshes() byte for byte, and both equal the numpy restatement (tests/glb_ref.py) -- with and without colours, under
simplify, smooth and clean, with an empty frame, a capacity too small, a re-run mesh, and in a ColorViewsSlot.  The
slots of the picture slot tests, the smallest ones.  Needs an MI355X."""
import numpy as np
import pytest

import glb_cases as cases
import glb_ref as ref
from test_color_views_slot_gpu import colour_slot, netc  # noqa: F401  (netc: the fixture)
from test_mesh_batch_gpu import BMAX, BMIN, DEV, nets  # noqa: F401  (nets: the fixture)
from test_slot_pictures_gpu import RES, frames, make_slot
from test_views_slot_gpu import frames as views_frames, net  # noqa: F401  (net: the fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def recon():
    from monoport_amd import recon as _recon
    return _recon


def restated(mesh, glb):
    """The file of a ``Mesh`` by the numpy restatement."""
    return ref.encode(mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), None,
                      mesh.normals.cpu().numpy() if glb.normals else None,
                      mesh.colors.cpu().numpy() if glb.colors else None, b_min=BMIN, b_max=BMAX)


def check_glbs(recon, slot, glb, live):
    files, meshes = slot.glbs(), slot.meshes()
    assert len(files) == len(meshes) == slot.n_active == len(live)
    for b, (f, mesh) in enumerate(zip(files, meshes)):
        if not live[b]:
            assert f is None and mesh is None
            continue
        assert isinstance(f, bytes) and mesh.verts.shape[0] > 30
        assert f == recon.encode_glb(mesh, glb, BMIN, BMAX) == restated(mesh, glb), b
        assert len(f) == ref.file_bytes(mesh.verts.shape[0], mesh.faces.shape[0], glb.normals, glb.colors)
        back = ref.Glb(f).mesh()  # and any reader gets the mesh, within the quantisation
        assert np.array_equal(back["faces"], mesh.faces.cpu().numpy())
        assert np.abs(back["positions"] - mesh.verts.cpu().numpy().astype(np.float64)).max() <= 0.52 * 2.0 / 65535
    return files


@pytest.mark.parametrize("colours", [True, False], ids=["colours", "plain"])
def test_slot_glbs(recon, nets, colours):  # noqa: F811
    images, calibs = frames()
    glb = recon.Glb(colors=colours)
    slot = make_slot(nets, {"normals": "accumulate"}, None, netc=colours)
    plain = make_slot(nets, {"normals": "accumulate"}, None, netc=colours)
    try:
        assert slot.glb is None and not hasattr(slot, "glb_bytes")
        slot.encode_meshes(glb)
        cap_v = 12 * RES[-1] ** 2
        assert slot.glb is glb and tuple(slot.glb_bytes.shape) == (2, glb.capacity_for(cap_v, 2 * cap_v))
        assert slot.glb_bytes.dtype == torch.uint8 and tuple(slot.glb_info.shape) == (2, 2)
        for s in (slot, plain):
            s.submit(images, calibs)
            s.wait()
        assert slot.status[:, 0].tolist() == [1, 0]
        assert plain.glb is None and not hasattr(plain, "glb_bytes") and not hasattr(plain, "glb_info")
        with pytest.raises(RuntimeError, match="before the first"):
            slot.encode_meshes(glb)
        with pytest.raises(RuntimeError, match="encode_meshes"):
            plain.glbs()
        files = check_glbs(recon, slot, glb, (True, False))
        info = slot.glb_info.cpu().numpy()
        assert tuple(info[0]) == (len(files[0]), 0) and tuple(info[1]) == (ref.MIN_BYTES, 0)  # the gated-off frame
        assert slot.glb_bytes[1, :ref.MIN_BYTES].cpu().numpy().tobytes() == cases.restated(cases.small_cases()[13])
        assert torch.equal(plain.meshes()[0].verts, slot.meshes()[0].verts)  # the chain is untouched
        if colours:  # the colours did arrive
            assert len(np.unique(ref.Glb(files[0]).mesh()["colors"])) > 10
        # a short batch behind it
        slot.submit(images[:1], calibs[:1])
        assert check_glbs(recon, slot, glb, (True,))[0] == files[0]
    finally:
        slot.close()
        plain.close()


@pytest.mark.parametrize("mesh", [{"simplify": 16}, {"smooth": 2}, {"clean": 6}], ids=["simplify16", "smooth2", "clean6"])
def test_slot_glbs_of_the_final_mesh(recon, nets, mesh):  # noqa: F811
    images, calibs = frames()
    glb = recon.Glb(colors=False)
    slot = make_slot(nets, dict(mesh, normals="accumulate", colors=False), None, netc=False)
    try:
        slot.encode_meshes(glb)
        slot.submit(images, calibs)
        check_glbs(recon, slot, glb, (True, False))
    finally:
        slot.close()


def test_a_capacity_too_small_and_a_mesh_made_again(recon, nets):  # noqa: F811
    images, calibs = frames()
    roomy = recon.Glb(colors=False)
    slot = make_slot(nets, {"normals": "accumulate", "colors": False}, None, netc=False)
    small = make_slot(nets, {"normals": "accumulate", "colors": False}, None, netc=False)
    try:
        slot.encode_meshes(roomy)
        slot.submit(images, calibs)
        files = check_glbs(recon, slot, roomy, (True, False))
        tight = recon.Glb(colors=False, capacity=len(files[0]) // 2)
        small.encode_meshes(tight)
        small.submit(images, calibs)
        small.wait()
        info = small.glb_info.cpu().numpy()
        assert tuple(info[0]) == (len(files[0]), 1) and tuple(info[1]) == (ref.MIN_BYTES, 0)
        assert small.glbs() == files
        assert recon.encode_glb(slot.meshes()[0], recon.Glb(colors=False, capacity=ref.MIN_BYTES), BMIN, BMAX) == files[0]
        # the mesh capacity cut behind the good submission: glbs() encodes the re-run mesh
        for k, v in slot.mesh_buffers.items():
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
        with torch.cuda.stream(slot.stream):
            slot._mesh_chain(2)
        slot._busy = True
        again = slot.glbs()
        assert slot._reran == [0] and again == files
        own = slot.glb_info.cpu().numpy()
        assert tuple(own[0]) == (ref.file_bytes(100, 200, True, False), 0)  # the truncated mesh's file
    finally:
        slot.close()
        small.close()


def test_color_views_slot_glbs(recon, net, netc):  # noqa: F811
    images, calibs = views_frames()
    glb = recon.Glb()
    slot = colour_slot(net, netc)
    try:
        slot.encode_meshes(glb)
        slot.submit(images, calibs)
        slot.wait()
        check_glbs(recon, slot, glb, (True, False))
    finally:
        slot.close()


def test_what_a_slot_refuses(recon, nets):  # noqa: F811
    from monoport_amd.pipeline import FramePipeline
    bare = make_slot(nets, None, None, netc=False)
    plain = make_slot(nets, {"normals": None, "colors": False}, None, netc=False)
    try:
        with pytest.raises(ValueError, match="without mesh"):
            bare.encode_meshes(recon.Glb())
        with pytest.raises(ValueError, match="recon.Glb"):
            plain.encode_meshes(recon.Jpeg())
        with pytest.raises(ValueError, match="normals"):
            plain.encode_meshes(recon.Glb(colors=False))
        with pytest.raises(ValueError, match="colors"):
            plain.encode_meshes(recon.Glb(normals=False))
        assert plain.glb is None and not hasattr(plain, "glb_bytes")
        plain.encode_meshes(recon.Glb(False, False, capacity=4096))
        assert tuple(plain.glb_bytes.shape) == (2, 4096)
    finally:
        bare.close()
        plain.close()
    pipe = FramePipeline(nets[0], torch.device(DEV), depth=1, batch=1, resolutions=RES, b_min=BMIN, b_max=BMAX,
                         mesh={"normals": "accumulate", "colors": False})
    try:
        glb = recon.Glb(colors=False)
        pipe.encode_meshes(glb)
        assert pipe.slots[0].glb is glb
    finally:
        pipe.close()


def test_encode_glb(recon):
    """Meshes of different sizes in one call, one of them empty; a capacity that two of them overflow."""
    made = [cases.random_mesh("a", 300, 515, 41, cases.SKEW), cases.random_mesh("b", 7, 3, 42, cases.SKEW),
            cases.random_mesh("c", 70, 0, 43, cases.SKEW), cases.random_mesh("d", 70, 90, 44, cases.SKEW)]
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    meshes = [recon.Mesh(t(c.verts), t(c.faces), t(c.normals), t(c.colors)) for c in made]
    for glb_kw in (dict(), dict(normals=False), dict(colors=False), dict(normals=False, colors=False)):
        glb = recon.Glb(**glb_kw)
        want = [cases.restated(c, glb.normals, glb.colors) for c in made]
        assert recon.encode_glb(meshes, glb, *cases.SKEW) == want
        tight = recon.Glb(capacity=len(want[1]) + 8, **glb_kw)
        assert recon.encode_glb(meshes, tight, *cases.SKEW) == want
    one = recon.encode_glb(meshes[1], None, *cases.SKEW)
    assert isinstance(one, bytes) and one == cases.restated(made[1])
    assert len(want[2]) == ref.MIN_BYTES
    bare = recon.Mesh(meshes[0].verts, meshes[0].faces, None, None)
    assert recon.encode_glb(bare, recon.Glb(False, False), *cases.SKEW) == cases.restated(made[0], False, False)
    with pytest.raises(ValueError, match="mesh 0 has no normals"):
        recon.encode_glb(bare)
