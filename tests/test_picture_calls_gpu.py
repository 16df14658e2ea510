"""Which C-ABI calls the pictures enqueue, on the GPU: a slot's ``_render_pictures``, the render call it is held to
(recon.render_mesh_many / render_mesh_many_in_scene on the slot's own meshes) and ``pictures()`` of a frame whose mesh
overflowed, each logged through ops.Context.check as a count per call name.  The counts below were recorded before the
three wirings became one body; none may grow, and a picture stage wired in twice shows as a count of 2: two frames of
two views are 4 pictures, at most ops.MAX_FRAMES, so every pass is one launch.  Needs an MI355X."""
import collections

import numpy as np
import pytest

from test_mesh_batch_gpu import nets  # noqa: F401  (the fixture)
from test_shadow_gpu import slot_scene
from test_slot_pictures_gpu import PICTURES, SIZE, TWO, frames, make_slot

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RENDER, CLIP = "mp_mesh_render_batch", "mp_mesh_render_clip_batch"
SCENE_WORDS = ("texture", "composite", "shadow", "light", "transfer", "volume_bits")
# config -> (mesh options, shade, over a lit scene, the Lighting's keywords or None, the slot runs netC)
CONFIGS = {
    "normals": ({"normals": "accumulate", "colors": False}, "normals", False, None, False),
    "netC": ({"normals": "accumulate", "colors": False}, "netC", False, None, True),
    "colors_scene": ({"normals": None}, "colors", True, None, True),
    "clay_transfer_scene": ({"normals": "accumulate", "colors": False}, "normals", True,
                            dict(albedo=(0.8, 0.7, 0.6), self_shadow=0.02, transfer=True), False),
    "netC_self_shadow_scene": ({"normals": "accumulate", "colors": False}, "netC", True, dict(self_shadow=0.02), True),
}
# recorded at the commit before the refactor: config -> (slot._render_pictures(2), the render call, pictures() of an
# overflowed frame).  The light's map is unclipped (a directional light), the pictures are clipped.
EXPECTED = {
    "normals": (
        {CLIP: 1},
        {CLIP: 1},
        {"mp_marching_cubes_batch": 1, "mp_mesh_normals_batch": 1, CLIP: 1}),
    "netC": (
        {CLIP: 1, "mp_picture_points_batch": 1, "mp_query_counted_batch_proj": 1, "mp_picture_paint_batch": 1},
        {"mp_feat_pack_hwc": 1, CLIP: 1, "mp_picture_points_batch": 1, "mp_query_counted": 1,
         "mp_picture_paint_batch": 1},
        {"mp_marching_cubes_batch": 1, "mp_mesh_normals_batch": 1, CLIP: 1, "mp_picture_points_batch": 1,
         "mp_query_counted": 1, "mp_picture_paint_batch": 1}),
    "colors_scene": (
        {CLIP: 3, RENDER: 1, "mp_picture_texture_batch": 1, "mp_picture_shadow_batch": 1,
         "mp_picture_composite_batch": 1},
        {CLIP: 3, RENDER: 1, "mp_picture_texture_batch": 1, "mp_picture_shadow_batch": 1,
         "mp_picture_composite_batch": 1},
        {"mp_marching_cubes_batch": 1, "mp_mesh_points_batch": 1, "mp_query_counted": 1, RENDER: 1, CLIP: 1,
         "mp_picture_shadow_batch": 1, "mp_picture_composite_batch": 1}),
    "clay_transfer_scene": (
        {RENDER: 1, CLIP: 6, "mp_mesh_transfer_batch": 1, "mp_picture_shadow_batch": 2,
         "mp_mesh_transfer_shade_batch": 1, "mp_picture_light_transfer_batch": 1, "mp_picture_texture_batch": 1,
         "mp_picture_composite_batch": 1},
        {RENDER: 1, CLIP: 6, "mp_picture_shadow_batch": 2, "mp_mesh_transfer_shade_batch": 1,
         "mp_picture_light_transfer_batch": 1, "mp_picture_texture_batch": 1, "mp_picture_composite_batch": 1},
        {"mp_marching_cubes_batch": 1, "mp_mesh_normals_batch": 1, "mp_mesh_transfer_batch": 1, RENDER: 1, CLIP: 4,
         "mp_picture_shadow_batch": 2, "mp_mesh_transfer_shade_batch": 1, "mp_picture_light_transfer_batch": 1,
         "mp_picture_composite_batch": 1}),
    "netC_self_shadow_scene": (
        {RENDER: 1, CLIP: 4, "mp_picture_shadow_batch": 2, "mp_picture_points_batch": 1,
         "mp_query_counted_batch_proj": 1, "mp_picture_paint_batch": 1, "mp_picture_light_batch": 1,
         "mp_picture_texture_batch": 1, "mp_picture_composite_batch": 1},
        {RENDER: 1, "mp_feat_pack_hwc": 1, CLIP: 4, "mp_picture_shadow_batch": 2, "mp_picture_points_batch": 1,
         "mp_query_counted": 1, "mp_picture_paint_batch": 1, "mp_picture_light_batch": 1,
         "mp_picture_texture_batch": 1, "mp_picture_composite_batch": 1},
        {"mp_marching_cubes_batch": 1, "mp_mesh_normals_batch": 1, RENDER: 1, CLIP: 2, "mp_picture_shadow_batch": 2,
         "mp_picture_points_batch": 1, "mp_query_counted": 1, "mp_picture_paint_batch": 1,
         "mp_picture_light_batch": 1, "mp_picture_composite_batch": 1}),
}


def _lighting(recon, kw):
    if kw is None:
        return None
    kw = dict(kw)
    if kw.pop("transfer", False):
        kw["transfer"] = recon.Transfer(64, reach=24)
    sh = np.random.RandomState(104).uniform(-0.6, 0.9, (9, 3)).astype(np.float32)
    return recon.Lighting(sh, direct=((0.3, -1.0, 0.2), (0.9, 0.8, 0.7)), **kw)


def _overflow(slot):
    """The slot's mesh chain and pictures again at 100 vertices / 200 faces, which frame 0 overflows."""
    for k, v in slot.mesh_buffers.items():
        if k in ("points", "preds"):  # channel-major [batch,3,cap]: fresh ones of the cut capacity
            slot.mesh_buffers[k] = torch.zeros((v.shape[0], 3, 100), dtype=v.dtype, device=v.device)
        else:
            slot.mesh_buffers[k] = {"verts": v[:, :100], "normals": v[:, :100], "faces": v[:, :200]}.get(k, v)
    with torch.cuda.stream(slot.stream):
        slot._mesh_chain(2)
        slot._render_pictures(2)
    slot._busy = True


@pytest.mark.parametrize("config", list(CONFIGS))
def test_picture_call_counts(nets, monkeypatch, config):  # noqa: F811
    from monoport_amd import ops, recon
    mesh, shade, in_scene, light_kw, netc = CONFIGS[config]
    scene = slot_scene(recon) if in_scene else None
    lighting = _lighting(recon, light_kw)
    pictures = dict(PICTURES, shade=shade)
    if scene is not None:
        pictures["scene"] = scene
    log = []
    real = ops.Context.check

    def check(self, rc, what):
        log.append(what)
        return real(self, rc, what)

    def logged(fn):
        torch.cuda.synchronize()
        del log[:]
        monkeypatch.setattr(ops.Context, "check", check)
        try:
            fn()
        finally:
            monkeypatch.setattr(ops.Context, "check", real)
        torch.cuda.synchronize()
        return dict(collections.Counter(log))

    images, calibs = frames()
    slot = make_slot(nets, mesh, pictures, netc=netc, lighting=lighting)
    try:
        slot.submit(images, calibs, cameras=TWO)
        slot.wait()

        def in_slot():
            with torch.cuda.stream(slot.stream):
                slot._render_pictures(2)

        got = [logged(in_slot)]
        meshes = slot.meshes()
        assert meshes[0] is not None and meshes[1] is None
        if lighting is not None and lighting.transfer is not None:
            meshes = [None if m is None else recon.with_transfer(m, recon.mesh_transfer(
                m, slot.volumes[b], lighting.transfer, slot.mesh.level, slot.b_min, slot.b_max)[0])
                for b, m in enumerate(meshes)]
        po = slot.picture_options
        kw = dict(projection=po.projection, nearest=po.nearest, background=po.background, near=po.near,
                  perspective_correct=po.perspective_correct, lighting=lighting)
        if shade == "netC":
            nchw = slot.feats_hwc_c[0].permute(2, 0, 1)[None].contiguous()
            kw.update(netC=slot.netC, feat_tensors_C=[[[nchw]], None], calib_tensors=[slot.calib[0:1], None])
        if scene is None:
            got.append(logged(lambda: recon.render_mesh_many(meshes, TWO, SIZE, shade, **kw)))
        else:
            got.append(logged(lambda: recon.render_mesh_many_in_scene(meshes, scene, TWO, SIZE, shade, **kw)))
        _overflow(slot)
        pics = []
        got.append(logged(lambda: pics.extend(slot.pictures())))
        assert slot._reran == [0] and len(pics) == 2
    finally:
        slot.close()
    print("%r: %r," % (config, tuple(got)))
    for counts in got:
        assert counts.get(RENDER, 0) + counts.get(CLIP, 0) >= 1
        if scene is None and lighting is None:  # nothing of a scene, a shadow, a light or a transfer without the option
            assert not [name for name in counts if any(w in name for w in SCENE_WORDS)], counts
    assert tuple(got) == EXPECTED[config]
