"""The numpy restatement of mp_picture_points / mp_picture_paint (tests/picture_ref.py) against the definition's own
words on small hand-made pictures, and the refusals of the Python layers of ``shade="netC"`` that need no device
(recon.render_mesh(_many), the slots' construction checks, the ops wrappers' argument checks)."""
import numpy as np
import pytest

import picture_ref as ref

torch = pytest.importorskip("torch")


def _picture(n_pixels, covered, seed=0):
    """face ids (-1 / a face index) and positions [L,3] whose every word is distinct."""
    rng = np.random.RandomState(seed)
    face = np.full(n_pixels, -1, np.int32)
    face[covered] = rng.randint(0, 1000, size=len(covered))
    pos = (np.arange(3 * n_pixels, dtype=np.float32).reshape(n_pixels, 3) + 0.25)
    return face, pos


def test_order_count_and_truncation():
    covered = [1, 4, 5, 9, 17, 18, 30]
    face, pos = _picture(31, covered)
    face[covered[2]] = 0  # face 0 is a face
    k_all = len(covered)
    for capacity in (k_all - 1, k_all, k_all + 1):
        pts = np.full((3, capacity), -7.0, np.float32)
        pix = np.full(capacity, -7, np.int32)
        got = ref.points(face, pos, capacity, pts, pix)
        n = min(k_all, capacity)
        assert got[0] is pts and got[1] is pix
        assert got[2].tolist() == [n, k_all] and got[2].dtype == np.int32
        assert pix[:n].tolist() == covered[:n]
        assert np.array_equal(pts[:, :n], pos[covered[:n]].T)
        assert (pts[:, n:] == -7.0).all() and (pix[n:] == -7).all()  # columns at or beyond count[0] are not written
        assert (got[2][1] > capacity) == (capacity == k_all - 1)  # how a caller detects truncation


def test_same_bits_not_same_values():
    face = np.array([0, -1, 3], np.int32)
    pos = np.array([[np.nan, -0.0, np.inf], [1, 2, 3], [1e-45, -np.inf, 0.0]], np.float32)
    pos.view(np.uint32)[0, 0] = 0x7FC12345  # a NaN with a payload
    pts, pix, count = ref.points(face, pos)
    assert count.tolist() == [2, 2] and pix.tolist() == [0, 2, 0]
    assert np.array_equal(pts.view(np.uint32)[:, :2], pos.view(np.uint32)[[0, 2]].T)


def test_none_and_all_covered():
    face, pos = _picture(12, [])
    pts, pix, count = ref.points(face, pos)
    assert count.tolist() == [0, 0] and not pts.any() and not pix.any()
    face, pos = _picture(12, list(range(12)))
    pts, pix, count = ref.points(face, pos)
    assert count.tolist() == [12, 12] and pix.tolist() == list(range(12)) and np.array_equal(pts, pos.T)
    face, pos = _picture(1, [0])
    assert ref.points(face, pos)[2].tolist() == [1, 1]


def test_paint_skips_what_lies_outside():
    values = np.array([[1.0, -1.0, 0.5, 3.0, 9.0], [0.0, 0.25, -3.0, 3.0, 9.0], [-0.5, 1.0, 1.0, 3.0, 9.0]], np.float32)
    pixels = np.array([2, -1, 6, 0, 4], np.int32)  # -1 and 6 lie outside an image of 6 pixels; entry 4 is beyond the count
    image = np.full((6, 3), 0.125, np.float32)
    out = ref.paint(values, pixels, np.array([4, 4], np.int32), image)
    assert out is image
    want = np.full((6, 3), 0.125, np.float32)
    want[2] = [1.0, 0.5, 0.25]
    want[0] = [2.0, 2.0, 2.0]
    assert np.array_equal(image, want)
    clamped = ref.paint(values, pixels, [4], np.full((6, 3), 0.125, np.float32), lo=0.0, hi=1.0)
    assert clamped[0].tolist() == [1.0, 1.0, 1.0] and clamped[2].tolist() == [1.0, 0.5, 0.25]
    # the count is clamped to [0, capacity]
    assert np.array_equal(ref.paint(values, pixels, [-3], np.full((6, 3), 0.125, np.float32)), np.full((6, 3), 0.125))
    far = ref.paint(values, pixels, [99], np.full((6, 3), 0.125, np.float32))
    assert far[4].tolist() == [5.0, 5.0, 5.0]
    # one rounding per operation: 0.1f * 3 + 0.1f in float32, not in double
    v = np.full((3, 1), 0.1, np.float32)
    got = ref.paint(v, np.zeros(1, np.int32), [1], np.zeros((1, 3), np.float32), scale=3.0, bias=0.1)
    assert got[0, 0] == np.float32(np.float32(0.1) * np.float32(3.0)) + np.float32(0.1)


def test_image_may_be_the_position_buffer():
    """points, then paint into the very array the positions were read from: covered pixels change, the others keep
    their positions' bits."""
    covered = [0, 3, 4, 10]
    face, pos = _picture(11, covered)
    before = pos.copy()
    pts, pix, count = ref.points(face, pos)
    values = -pts  # what a query might answer
    ref.paint(values, pix, count, pos)
    rest = [p for p in range(11) if p not in covered]
    assert np.array_equal(pos[rest], before[rest])
    assert np.array_equal(pos[covered], before[covered] * np.float32(-0.5) + np.float32(0.5))


# ---- the Python layers' refusals ------------------------------------------------------------------------------------

def _net(kind, v_n):
    from monoport_amd.modeling import PIFuNetC, PIFuNetG, heads
    net = PIFuNetG() if kind == "G" else PIFuNetC()
    ch = [257, 1024, 512, 256, 128, 1] if kind == "G" else [513, 1024, 512, 256, 128, 3]
    net.surface_classifier = heads.SurfaceClassifier(ch, v_n, False, "sigmoid" if kind == "G" else "tanh")
    return net.eval()


def _mesh():
    from monoport_amd.recon import Mesh
    verts = torch.tensor([[0.0, 0, 0], [0.5, 0, 0], [0, 0.5, 0]])
    return Mesh(verts, torch.tensor([[0, 1, 2]], dtype=torch.int32), None, None)


def test_render_mesh_refusals():
    from monoport_amd import recon
    assert "netC" in recon.SHADES
    eye = torch.eye(4)
    for mesh in (_mesh(), None):  # refused before anything else is looked at, a None mesh included
        with pytest.raises(ValueError, match="netC"):
            recon.render_mesh(mesh, eye, 8, shade="netC")
        for shade in ("colors", "normals", None):
            with pytest.raises(ValueError, match="netC"):
                recon.render_mesh(mesh, eye, 8, shade=shade, netC=_net("C", 1))
        with pytest.raises(ValueError, match="multi-view"):  # view= picks a row of a multi-view head
            recon.render_mesh(mesh, eye, 8, shade="netC", netC=_net("C", 1), view=0)
        with pytest.raises(ValueError, match="view must be"):
            recon.render_mesh(mesh, eye, 8, shade="netC", netC=_net("C", 2), view=2)
    with pytest.raises(ValueError, match="no netC"):
        recon.render_mesh(_mesh(), eye, 8, shade=None, view=0)
    with pytest.raises(ValueError, match="netC"):
        recon.render_mesh_many([_mesh(), None], eye, 8, shade="netC")
    with pytest.raises(ValueError, match="feat_tensors_C"):
        recon.render_mesh_many([_mesh()], eye, 8, shade="netC", netC=_net("C", 1))
    with pytest.raises(ValueError, match="2 meshes, 1 feature sets"):
        recon.render_mesh_many([_mesh(), None], eye, 8, shade="netC", netC=_net("C", 1), feat_tensors_C=[None],
                               calib_tensors=[None, None])
    with pytest.raises(NotImplementedError, match="view="):  # a multi-view head without view=
        recon.render_mesh(_mesh(), eye, 8, shade="netC", netC=_net("C", 2), feat_tensor_C=[[torch.zeros(2, 512, 4, 4)]],
                          calib_tensor=torch.eye(4)[None].repeat(2, 1, 1))
    # nothing of this reached a device: a list of None meshes with a well-formed request returns Nones
    assert recon.render_mesh_many([None, None], eye, 8, shade="netC", netC=_net("C", 1), feat_tensors_C=[None, None],
                                  calib_tensors=[None, None]) == [None, None]


def test_slot_refusals():
    from monoport_amd import pipeline
    mesh = {"normals": None, "colors": False}
    with pytest.raises(ValueError, match="netC"):  # a slot without netC has nothing to query per pixel
        pipeline.FrameSlot(_net("G", 1), "cpu", mesh=mesh, pictures={"shade": "netC"})
    with pytest.raises(ValueError, match="mesh="):  # the pictures are of the slot's meshes
        pipeline.FrameSlot(_net("G", 1), "cpu", netC=_net("C", 1), pictures={"shade": "netC"})
    with pytest.raises(ValueError, match="netC"):  # a plain ViewsSlot runs no netC
        pipeline.ViewsSlot(_net("G", 2), "cpu", mesh=mesh, pictures={"shade": "netC"})
    with pytest.raises(NotImplementedError, match="netC"):
        pipeline.ViewsSlot(_net("G", 2), "cpu", netC=_net("C", 2), mesh=mesh, pictures={"shade": "netC"})
    # the option itself passes the checks, and needs no colours on the mesh
    po = pipeline._picture_options({"shade": "netC", "views": 2, "res": (40, 24)},
                                   pipeline._mesh_options(mesh, 0.5, True), True)
    assert po.shade == "netC" and po.views == 2 and po.res == (40, 24)
    with pytest.raises(ValueError, match="shade"):
        pipeline._picture_options({"shade": "netc"}, pipeline._mesh_options(mesh, 0.5, True), True)


def test_ops_wrappers_check_their_lists_before_any_device_work():
    from monoport_amd import ops
    face, pos = torch.zeros(6, dtype=torch.int32), torch.zeros(6, 3)
    for bad_face, bad_pos in ((face.long(), pos), (face, pos.double()), (face, pos[:5]), (face[::2], pos[:3]),
                              (torch.zeros(0, dtype=torch.int32), torch.zeros(0, 3))):
        with pytest.raises(ValueError, match="picture_points"):
            ops.picture_points(bad_face, bad_pos)
    with pytest.raises(ValueError, match="capacity"):
        ops.picture_points(face, pos, capacity=0)
    with pytest.raises(ValueError, match="picture_points_batch"):
        ops.picture_points_batch([face, face], [pos])
    with pytest.raises(ValueError, match=r"out\[1\]"):
        ops.picture_points(face, pos, out=(torch.zeros(3, 6), torch.zeros(5, dtype=torch.int32),
                                           torch.zeros(2, dtype=torch.int32)))
    values, pixels, count = torch.zeros(3, 4), torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="n_pixels"):
        ops.picture_paint(values, pixels, count)
    for bad in (dict(values=values.t().contiguous()), dict(pixels=pixels.long()), dict(pixels=pixels[:3]),
                dict(count=count.float()), dict(out=torch.zeros(6, 3).double()), dict(out=torch.zeros(7))):
        args = dict(values=values, pixels=pixels, count=count, out=pos.clone())
        args.update(bad)
        with pytest.raises(ValueError, match="picture_paint"):
            ops.picture_paint(args["values"], args["pixels"], args["count"], out=args["out"])
    with pytest.raises(ValueError, match="picture_paint_batch"):
        ops.picture_paint_batch([values], [pixels, pixels], [count], out=[pos.clone()])
    with pytest.raises(ValueError, match="face ids"):
        ops.render_netc_batch("who", [], [], [], [], ops.raster("who", 8), None, out=(torch.zeros(1), None, None))
