"""The coloured mesh of the 257^3 body volume, three ways in ONE process on one MI355X:

  (a) recon.marching_cubes + mesh_util.vertex_colors  (two host round trips: the counts, then the colour query)
  (b) recon.reconstruct_mesh(normals=None, netC=...)   (one device chain, one host sync)
  (c) recon.reconstruct_mesh(normals="accumulate", netC=...)   ((b) plus the per-vertex normals)
  (d) as (c) with normals="reference"

    python tools/mesh_timing.py [--passes 5] [--meshes 20] [--out profiles/mesh_timing.json]

``--batched`` measures the batched chain instead (profiles/mesh_batch_timing.json): on the same volume and netC, at
n = 4 and n = 20 meshes, n calls of recon.reconstruct_mesh against ONE recon.reconstruct_mesh_many, with and without
colours (normals="accumulate" in both), per-mesh milliseconds; and a pipeline.FrameSlot(mesh=...) of 20 frames
(encoders as a hipGraph, netC, the bench's synthetic frames) with pipeline.MESH_BATCH at 1 / 4 / all frames, alone and
as three slots submitted back to back, per-frame milliseconds -- next to the same slots without mesh output, and to
the mesh slot with ``pictures`` (4 clipped, perspective-correct views per frame at 257^2, normals shading;
``pictures()`` included).

    python tools/mesh_timing.py --batched [--passes 5] [--out profiles/mesh_batch_timing.json]

``--clean`` measures what keeping the largest connected body costs (profiles/keep_largest_timing.json): on the same
volume with three planted floaters, recon.keep_largest alone and per frame of one recon.keep_largest_many of 20 (both
connectivities), ops.marching_cubes_raw alone (the stage cleaning precedes), recon.reconstruct_mesh and
recon.reconstruct_mesh_many of 20 with netC colours without / with clean=6; and the 20-frame colour slot of ``--batched``
with a mesh per frame without / with ``"clean": 6``.  ``--clean --no-slot`` leaves the slot out.

    python tools/mesh_timing.py --clean [--passes 5] [--out profiles/keep_largest_timing.json]

``--render`` measures the mesh rasteriser (profiles/mesh_render_timing.json): on the same volume's mesh (normals
shading), recon.render_mesh / render_mesh_many at 257^2 and 1024^2, 1 and 4 cameras, 1 and 20 meshes per call, in
milliseconds per picture; beside them the existing way to one picture of the volume (ops.forward_vertices_raw +
ops.paint, one axis direction at the volume's resolution) and what one more reconstruction of the volume costs (what a
second view cost before).

    python tools/mesh_timing.py --render [--passes 5] [--out profiles/mesh_render_timing.json]

``--render --clip`` adds, in the same passes, the clipped form (profiles/mesh_render_clip_timing.json): the same mesh at
257^2 under a perspective camera that has the whole body in front of it, through the unclipped call, through
``near=0.5`` (the same picture, so the difference is the price of the extra setup store and the classification) without
and with ``perspective_correct``, and with the plane through the body (``near=3.0``); 1 and 20 meshes per call.

    python tools/mesh_timing.py --render --clip [--passes 5] [--out profiles/mesh_render_clip_timing.json]

``--simplify`` measures the level-of-detail dial (profiles/mesh_simplify_timing.json): on the same volume,
recon.reconstruct_mesh_many of 20 meshes with and without netC colours, and the 20-frame colour slot of ``--batched``
with a mesh per frame, each at ``simplify`` None / 128 / 64 (normals="accumulate"), per-mesh / per-frame milliseconds,
with the vertex and face counts at each setting.  ``--simplify --no-slot`` leaves the slot out.

    python tools/mesh_timing.py --simplify [--passes 5] [--out profiles/mesh_simplify_timing.json]

``--smooth`` measures the Taubin passes (profiles/mesh_smooth_timing.json): on the same volume,
recon.reconstruct_mesh_many of 20 meshes without colours, with netC colours, and with colours behind ``simplify=128``,
each at ``smooth`` None / 2 / 10 (normals="accumulate"), per-mesh milliseconds, with the launches that one smoothing
call enqueues (4 + 2 x iterations kernels and one memset, whatever the number of meshes up to ops.MAX_FRAMES).  The
comparison is the ``smooth=None`` rows of the same run.

    python tools/mesh_timing.py --smooth [--passes 5] [--out profiles/mesh_smooth_timing.json]

``--deferred`` measures pictures coloured per pixel (profiles/mesh_deferred_timing.json): 20-frame colour slots on
the 257^3 body, in one session with alternating passes, (a) colours on the mesh and ``shade="colors"`` at 257^2 with 1
view -- the per-vertex colour query -- against (b) ``"colors": False`` and ``shade="netC"`` -- netC at the covered pixels
only -- at 257^2 with 1 view, at 257^2 with 4 views and at 1024^2 with 1 view, per-frame milliseconds of a submission
(``pictures()`` included), with the covered pixels per picture beside the vertex count.  The cameras are turned off the
axes.

    python tools/mesh_timing.py --deferred [--passes 5] [--out profiles/mesh_deferred_timing.json]

``--scene`` measures the scene behind the subject (profiles/mesh_scene_timing.json): 20-frame slots on the 257^3 body
with normal-shaded pictures under a free perspective camera (near plane, perspective-correct), in one session with
alternating passes, without and with ``scene=`` -- a 3 m floor of two triangles textured with a 2048^2 checker, full
mip chain, composited by depth -- at one 257^2 and one 1024^2 view, per-frame milliseconds of a submission
(``pictures()`` included), with the composite's mask counts of frame 0.  The rows without the scene are the comparison.

    python tools/mesh_timing.py --scene [--passes 5] [--out profiles/mesh_scene_timing.json]

``--shadow`` measures the subject's shadow on that scene (profiles/mesh_shadow_timing.json): the ``--scene`` set-up, the
slots WITH the scene, each without and with ``light=`` on it -- ``Light.directional`` from above and the side, fitted to
the scene's box, a 512^2 map, radius 1 -- at one 257^2 and one 1024^2 view, with the shadowed pixels of frame 0.  The
rows without a light are the comparison.

    python tools/mesh_timing.py --shadow [--passes 5] [--out profiles/mesh_shadow_timing.json]

``--lighting`` measures the per-pixel lighting of the subject (profiles/mesh_lighting_timing.json): the ``--shadow``
slots WITH the light on the scene, each without and with ``lighting=`` -- clay albedo, random second-order SH
coefficients, a direct term along the sun, evaluated in the camera's frame, with the self-shadow (bias 0.02) -- at one
257^2 and one 1024^2 view, with the subject's pixels of frame 0 that the lighting changes.  The rows without
``lighting=`` are the comparison.

    python tools/mesh_timing.py --lighting [--passes 5] [--out profiles/mesh_lighting_timing.json]

``--transfer`` measures the self-occluded SH term (profiles/mesh_transfer_timing.json): per mesh in a batch of 20 on
the 257^3 body, the occupancy bits, the radiance transfer and its shade each alone at D = 64, 128 and 256 directions,
with the samples the definition visits per second and the share of them that lie in empty 8^3 blocks (what the
tracer may skip); then the ``--lighting`` slots (without the self-shadow, SH in the world frame) without and with
``transfer=`` at one 257^2 and one 1024^2 view, alternated in one session.

    python tools/mesh_timing.py --transfer [--passes 5] [--out profiles/mesh_transfer_timing.json]

``--jpeg`` measures the pictures' encoding (profiles/mesh_jpeg_timing.json): mp_picture_jpeg alone, per picture in a
batch of 20 lit pictures at 257^2 and 1024^2, quality 90, 420 and 444, with the median file size; then the
``--lighting`` slots without and with ``encode_pictures``, with ``pictures()`` against ``jpegs()`` as the consumer, and,
where Pillow is importable, the way to a JPEG without it: ``pictures()``, ``.cpu()``, Pillow ``save``.

    python tools/mesh_timing.py --jpeg [--passes 5] [--out profiles/mesh_jpeg_timing.json]

``--png`` measures the lossless encoding (profiles/mesh_png_timing.json): mp_picture_png alone, per picture in a batch
of 20 lit pictures at 257^2 and 1024^2 for 8-bit RGB, 8-bit RGBA (the subject's mask as alpha) and the 16-bit depth, with
the median file size; then the 20-frame lit slot with ``pngs()`` as the consumer against ``pictures()``, ``.cpu()`` and
Pillow ``save(compress_level=6)`` on the host, alternated in one session.

    python tools/mesh_timing.py --png [--passes 5] [--out profiles/mesh_png_timing.json]

``--samples`` measures anti-aliasing (profiles/mesh_samples_timing.json): mp_picture_resolve_batch alone, per picture
in a batch of 20 composited pictures (image, depth, face ids and mask in; all five planes out) at the final sizes 257^2
and 1024^2 for ``samples`` = 2 and 4, with the achieved GB/s (bytes read plus bytes written), beside a device-to-device
copy that moves the same number of bytes, timed in the same alternating passes; then the ``--jpeg`` slots (the floor
with its light, clay lighting with the self-shadow, ``encode_pictures``, ``jpegs()`` as the consumer) at ``samples``
absent / 2 / 4 with one 257^2 view and absent / 2 with one 1024^2 view (4096 is the size limit).

    python tools/mesh_timing.py --samples [--passes 5] [--out profiles/mesh_samples_timing.json]

``--glb`` measures the meshes' way out (profiles/mesh_glb_timing.json): mp_mesh_glb_batch alone, per mesh in a batch of
20 coloured meshes of the 257^3 body at simplify = None / 128 / 64, with the file size and the achieved GB/s (bytes read
plus bytes written), beside a device-to-device copy that moves the same number of bytes and beside the host route it
replaces (the tensors' ``.cpu()`` and the numpy packing of tests/glb_ref.py), in the same alternating passes; then the
20-frame colour slot with a mesh per frame, ``meshes()`` against ``glbs()`` as the consumer and against ``meshes()``,
``.cpu()`` and the numpy packing.

    python tools/mesh_timing.py --glb [--passes 5] [--out profiles/mesh_glb_timing.json]

``--texture`` measures the textured way out (profiles/mesh_texture_timing.json): 20-frame colour slots with a mesh per
frame of the 257^3 body at ``simplify=64``, ``glbs()`` as the consumer: with COLOR_0 (``recon.Glb()``), with
``recon.Glb(texture=recon.Atlas(1024, 8))`` and with ``Atlas(2048, 16)`` (whose slots run no per-vertex colour query), and
the same textured file made through the host: ``meshes()``, ``.cpu()`` of the tensors and of netC's bake, the numpy
restatement's writer (tests/glb_texture_ref.py) and Pillow's PNG encoder.  It states the texels queried per frame.

    python tools/mesh_timing.py --texture [--passes 5] [--out profiles/mesh_texture_timing.json]

The protocol of tools/recon_views_timing.py: after a warm-up of all, the passes alternate; a pass is `meshes`
meshes, wall clock around a final stream sync.  Prints (and writes) one JSON line: per way the median, minimum and
maximum time per mesh (ms) over the passes.  The verdict fields restate what to check: (b) not slower than (a) by
more than the larger min-max spread of the two, and what the normals add to (b).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monoport_amd import mesh_util, ops, synthetic as syn  # noqa: E402
from monoport_amd.modeling import PIFuNetC  # noqa: E402
from monoport_amd import recon  # noqa: E402
from monoport_amd.recon import marching_cubes, reconstruct_mesh, reconstruct_mesh_many  # noqa: E402
from oracle import pifu_oracle as orc  # noqa: E402

DEV = "cuda:0"
RES = [17, 33, 65, 129, 257]
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--meshes", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batched", action="store_true", help="the batched chain and the slot's MESH_BATCH settings")
    ap.add_argument("--clean", action="store_true", help="what keeping the largest connected body costs")
    ap.add_argument("--no-slot", action="store_true", help="with --clean / --simplify: leave the frame slot out")
    ap.add_argument("--simplify", action="store_true", help="the mesh chain at simplify = None / 128 / 64")
    ap.add_argument("--smooth", action="store_true", help="the mesh chain at smooth = None / 2 / 10")
    ap.add_argument("--render", action="store_true", help="the mesh rasteriser against the visible-surface picture")
    ap.add_argument("--clip", action="store_true", help="with --render: the clipped form beside the unclipped call")
    ap.add_argument("--deferred", action="store_true", help="slot pictures coloured per vertex against per pixel")
    ap.add_argument("--scene", action="store_true", help="slot pictures with and without a textured scene behind them")
    ap.add_argument("--shadow", action="store_true", help="slot pictures over a scene, without and with a light on it")
    ap.add_argument("--lighting", action="store_true", help="the --shadow slots without and with lighting= on the subject")
    ap.add_argument("--transfer", action="store_true", help="bits, transfer and shade per mesh; lit slots with transfer=")
    ap.add_argument("--jpeg", action="store_true", help="mp_picture_jpeg alone; the --lighting slots with encode_pictures")
    ap.add_argument("--png", action="store_true", help="mp_picture_png alone; the --lighting slots with a recon.Png")
    ap.add_argument("--samples", action="store_true", help="mp_picture_resolve alone; the --jpeg slots at samples 1 / 2 / 4")
    ap.add_argument("--glb", action="store_true", help="mp_mesh_glb_batch alone; the colour slot with encode_meshes")
    ap.add_argument("--texture", action="store_true", help="the colour slot's glbs() with COLOR_0 against a baked atlas")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "mesh_texture_timing.json" if a.texture else
                             "mesh_render_clip_timing.json" if a.render and a.clip else
                             "mesh_render_timing.json" if a.render else
                             "mesh_deferred_timing.json" if a.deferred else
                             "mesh_scene_timing.json" if a.scene else
                             "mesh_shadow_timing.json" if a.shadow else
                             "mesh_lighting_timing.json" if a.lighting else
                             "mesh_transfer_timing.json" if a.transfer else
                             "mesh_jpeg_timing.json" if a.jpeg else
                             "mesh_png_timing.json" if a.png else
                             "mesh_samples_timing.json" if a.samples else
                             "mesh_glb_timing.json" if a.glb else
                             "mesh_smooth_timing.json" if a.smooth else
                             "mesh_simplify_timing.json" if a.simplify else
                             "keep_largest_timing.json" if a.clean else
                             "mesh_batch_timing.json" if a.batched else "mesh_timing.json")
    if a.texture:
        write(a, slot_texture(a))
        return
    if a.deferred:
        write(a, slot_deferred(a))
        return
    if a.scene:
        write(a, slot_scene(a))
        return
    if a.shadow:
        write(a, slot_shadow(a))
        return
    if a.lighting:
        write(a, slot_lighting(a))
        return
    if a.jpeg:
        write(a, slot_jpeg(a))
        return
    if a.png:
        write(a, slot_png(a))
        return
    if a.samples:
        out = resolve_kernels(a)
        if not a.no_slot:
            out["slot"] = slot_samples(a)
        write(a, out)
        return
    if a.transfer:
        out = transfer_kernels(a)
        if not a.no_slot:
            out["slot"] = slot_transfer(a)
        write(a, out)
        return
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    fh = ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2))[None].to(DEV))
    cal = torch.from_numpy(orc.pifu_calib(*syn.scene_camera(30))).to(DEV)
    vol, status = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES)
    assert int(status[0].item()) == 1
    vol = vol[None, None]
    if a.render:
        write(a, render(a, vol, lambda: ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES)))
        return
    netC = PIFuNetC()
    with torch.no_grad():
        for i, (w, b) in enumerate(syn.rand_mlp("C", 61, 2.0)):
            netC.surface_classifier.filters[i].weight.copy_(torch.from_numpy(w)[:, :, None])
            netC.surface_classifier.filters[i].bias.copy_(torch.from_numpy(b))
    netC.surface_classifier.to(DEV)
    netC.eval()
    feat_C = [[torch.from_numpy(syn.rand_feat(512, 128, 128, 62))[None].to(DEV)]]
    calib = torch.eye(4, device=DEV)[None]

    if a.smooth:
        write(a, smooth(a, vol, netC, feat_C, calib))
        return
    if a.glb:
        out = glb_kernels(a, vol, netC, feat_C, calib)
        if not a.no_slot:
            out["slot"] = slot_glb(a)
        write(a, out)
        return
    if a.simplify:
        out = simplify(a, vol, netC, feat_C, calib)
        if not a.no_slot:
            out["slot"] = slot_simplify(a)
        write(a, out)
        return
    if a.clean:
        out = clean(a, vol, netC, feat_C, calib)
        if not a.no_slot:
            out["slot"] = slot_clean(a)
        write(a, out)
        return
    if a.batched:
        out = batched(a, vol, netC, feat_C, calib)
        out["slot"] = slot_mesh_batch(a)
        write(a, out)
        return

    def two_calls():
        verts, faces = marching_cubes(vol, 0.5, BMIN, BMAX)
        return verts, faces, None, mesh_util.vertex_colors(netC, feat_C, verts, calib)

    def chain(normals):
        return lambda: reconstruct_mesh(vol, 0.5, BMIN, BMAX, normals=normals, netC=netC, feat_tensor_C=feat_C,
                                        calib_tensor=calib)

    ways = {"two_calls": two_calls, "chain": chain(None), "chain_normals": chain("accumulate"),
            "chain_normals_reference": chain("reference")}

    def run(name, n):
        for _ in range(n):
            out = ways[name]()
        return out

    first = {name: run(name, 3) for name in ways}  # warm-up of all
    torch.cuda.synchronize()
    same = all(torch.equal(first[name][0], first["two_calls"][0]) and torch.equal(first[name][1], first["two_calls"][1])
               and torch.equal(first[name][3], first["two_calls"][3]) for name in ways)
    times = {name: [] for name in ways}
    for _ in range(a.passes):
        for name in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, a.meshes)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.meshes)
    out = {"resolutions": RES, "vertices": int(first["chain"][0].shape[0]), "faces": int(first["chain"][1].shape[0]),
           "passes": a.passes, "meshes_per_pass": a.meshes, "meshes_and_colours_equal": bool(same)}
    for name in ways:
        t = np.array(times[name])
        out[name] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                     "max_ms": round(float(t.max()), 4)}
    spread = max(out[n]["max_ms"] - out[n]["min_ms"] for n in ("two_calls", "chain"))
    out["larger_spread_ms"] = round(spread, 4)
    out["chain_not_slower_than_two_calls_by_more_than_spread"] = bool(
        out["chain"]["median_ms"] <= out["two_calls"]["median_ms"] + spread)
    out["normals_add_ms"] = round(out["chain_normals"]["median_ms"] - out["chain"]["median_ms"], 4)
    out["reference_normals_add_ms"] = round(out["chain_normals_reference"]["median_ms"] - out["chain"]["median_ms"], 4)
    write(a, out)


def write(a, out):
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh_:
        fh_.write(line + "\n")


def stats(ms):
    t = np.array(ms)
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
            "max_ms": round(float(t.max()), 4)}


def alternate(ways, passes, per):
    """Warm-up of all, then ``passes`` alternating passes: wall clock around a final device sync, per ``per`` items."""
    for fn in ways.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in ways}
    for _ in range(passes):
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / per)
    return {name: stats(t) for name, t in times.items()}


def batched(a, vol, netC, feat_C, calib):
    """n x reconstruct_mesh against one reconstruct_mesh_many, per-mesh ms, with and without colours."""
    out = {"resolutions": RES, "passes": a.passes, "normals": "accumulate", "unit": "ms per mesh"}
    for n in (4, 20):
        def calls(colour):
            kw = dict(netC=netC, feat_tensor_C=feat_C, calib_tensor=calib) if colour else {}
            return lambda: [reconstruct_mesh(vol, 0.5, BMIN, BMAX, **kw) for _ in range(n)]

        def many(colour):
            kw = dict(netC=netC, feat_tensors_C=[feat_C] * n, calib_tensors=[calib] * n) if colour else {}
            return lambda: reconstruct_mesh_many([vol] * n, 0.5, BMIN, BMAX, **kw)

        ways = {"calls_colours": calls(True), "many_colours": many(True), "calls": calls(False), "many": many(False)}
        one, all_ = ways["calls_colours"]()[0], ways["many_colours"]()
        same = all(torch.equal(x, y) for m in all_ for x, y in zip(m, one))
        res = alternate(ways, a.passes, n)
        res["equal"] = bool(same)
        res["many_over_calls_colours"] = round(res["many_colours"]["median_ms"] / res["calls_colours"]["median_ms"], 4)
        res["many_over_calls"] = round(res["many"]["median_ms"] / res["calls"]["median_ms"], 4)
        out["n%d" % n] = res
        out["vertices"], out["faces"] = int(one.verts.shape[0]), int(one.faces.shape[0])
    return out


def render(a, vol, reconstruct, n=20):
    """Milliseconds per picture of the mesh rasteriser, of forward_vertices + paint and of one more reconstruction."""
    mesh = reconstruct_mesh(vol, 0.5, BMIN, BMAX, normals="accumulate")
    cams = torch.cat([torch.eye(4)[None]] + [recon.pifu_calib(*syn.scene_camera(30 * k), device="cpu")
                                             for k in (1, 2, 3)])
    r = vol.shape[-1]

    def surface_picture():
        for _ in range(n):
            x, y, _, norm, count = ops.forward_vertices_raw(vol, "front")
            ops.paint(x, y, norm, False, count, r, 0.5, 0.5, 0.0, 1.0)

    ways = {"forward_vertices_paint_%d" % r: surface_picture,
            "reconstruction": lambda: [reconstruct() for _ in range(n)]}
    per = {name: n for name in ways}
    for size in (257, 1024):
        for views in (1, 4):
            c = cams[0] if views == 1 else cams[:views]
            name = "render_%d_views%d" % (size, views)
            ways[name + "_frames1"] = (lambda c=c, size=size: [
                recon.render_mesh(mesh, c, res=size, shade="normals") for _ in range(n)])
            ways[name + "_frames%d" % n] = (lambda c=c, size=size: recon.render_mesh_many(
                [mesh] * n, c, res=size, shade="normals"))
            per[name + "_frames1"] = per[name + "_frames%d" % n] = n * views
    out = {"resolutions": RES, "passes": a.passes, "unit": "ms per picture", "shade": "normals",
           "vertices": int(mesh.verts.shape[0]), "faces": int(mesh.faces.shape[0]), "pictures_per_pass": per}
    if a.clip:
        out["clip"] = clip_ways(mesh, ways, per, n)
    one = recon.render_mesh(mesh, cams[0], res=r, shade="normals")
    x, y, _, _ = recon.forward_vertices(vol, "front")
    seen = torch.zeros((r, r), dtype=torch.bool, device=vol.device)
    seen[x, y] = True
    out["silhouette_pixels"] = int(seen.sum().item())
    out["silhouette_differs_from_forward_vertices"] = int(((one.face >= 0) != seen).sum().item())
    for fn in ways.values():  # warm-up of all
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in ways}
    for _ in range(a.passes):
        for name, fn in ways.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / per[name])
            del res
    out.update({name: stats(t) for name, t in times.items()})
    return out


def clip_ways(mesh, ways, per, n):
    """Adds the perspective rows of ``--clip`` to ``ways`` / ``per``; returns what they draw."""
    cam = torch.eye(4)
    cam[0, 0] = cam[1, 1] = 2.5
    cam[2, 3] = 3.0  # the box [-1, 1]^3 at z = 2 .. 4
    rows = {"persp": {}, "persp_clip": dict(near=0.5), "persp_clip_correct": dict(near=0.5, perspective_correct=True),
            "persp_cut": dict(near=3.0), "persp_cut_correct": dict(near=3.0, perspective_correct=True)}

    def one(kw):
        return recon.render_mesh(mesh, cam, res=257, shade="normals", projection="perspective", nearest="min", **kw)

    for name, kw in rows.items():
        ways[name + "_257_frames1"] = (lambda kw=kw: [one(kw) for _ in range(n)])
        ways[name + "_257_frames%d" % n] = (lambda kw=kw: recon.render_mesh_many(
            [mesh] * n, cam, res=257, shade="normals", projection="perspective", nearest="min", **kw))
        per[name + "_257_frames1"] = per[name + "_257_frames%d" % n] = n
    pics = {name: one(kw) for name, kw in rows.items()}
    return {"camera": "focal 2.5 at z = 3: the body at 2 .. 4", "near_in_front": 0.5, "near_through_the_body": 3.0,
            "clip_in_front_equals_unclipped": all(torch.equal(x, y) for x, y in zip(pics["persp"], pics["persp_clip"])),
            "covered_pixels": {name: int((p_.face >= 0).sum().item()) for name, p_ in pics.items()}}


def clean(a, vol, netC, feat_C, calib, n=20):
    """keep_largest alone and batched, marching cubes alone, and the mesh calls without / with clean=6."""
    dirty = vol.clone()
    for k, (z, y, x, h) in enumerate(((12, 12, 12, 4), (240, 30, 200, 3), (20, 236, 128, 2))):  # three floaters
        dirty[0, 0, z:z + h, y:y + h, x:x + h] = 0.9
    stats = {c: ops.keep_largest_raw(dirty, 0.5, c, 0.0)[1].cpu().tolist() for c in (6, 26)}
    kw = dict(netC=netC, feat_tensor_C=feat_C, calib_tensor=calib)
    kwn = dict(netC=netC, feat_tensors_C=[feat_C] * n, calib_tensors=[calib] * n)
    ways = {
        "keep_largest_6": lambda: [recon.keep_largest(dirty, 0.5, 6) for _ in range(n)],
        "keep_largest_26": lambda: [recon.keep_largest(dirty, 0.5, 26) for _ in range(n)],
        "keep_largest_many_6": lambda: recon.keep_largest_many([dirty] * n, 0.5, 6),
        "keep_largest_many_26": lambda: recon.keep_largest_many([dirty] * n, 0.5, 26),
        "marching_cubes_raw": lambda: [ops.marching_cubes_raw(dirty, 0.5, BMIN, BMAX) for _ in range(n)],
        "marching_cubes_raw_batch": lambda: ops.marching_cubes_raw_batch([dirty] * n, 0.5, BMIN, BMAX),
        "mesh": lambda: [reconstruct_mesh(dirty, 0.5, BMIN, BMAX, **kw) for _ in range(n)],
        "mesh_clean": lambda: [reconstruct_mesh(dirty, 0.5, BMIN, BMAX, clean=6, **kw) for _ in range(n)],
        "mesh_many": lambda: reconstruct_mesh_many([dirty] * n, 0.5, BMIN, BMAX, **kwn),
        "mesh_many_clean": lambda: reconstruct_mesh_many([dirty] * n, 0.5, BMIN, BMAX, clean=6, **kwn),
    }
    one, cleaned = ways["mesh"]()[0], ways["mesh_clean"]()[0]
    out = {"resolutions": RES, "passes": a.passes, "per_pass": n, "unit": "ms per volume / mesh",
           "stats_6": stats[6], "stats_26": stats[26], "vertices": int(one.verts.shape[0]),
           "vertices_clean": int(cleaned.verts.shape[0])}
    out.update(alternate(ways, a.passes, n))
    for name in ("mesh", "mesh_many"):
        out[name + "_clean_adds_ms"] = round(out[name + "_clean"]["median_ms"] - out[name]["median_ms"], 4)
    return out


def slot_clean(a, frames=20):
    """The 20-frame colour slot with a mesh per frame, without and with "clean": 6, per-frame ms of a submission
    (``meshes()`` included)."""
    pipes, fn = _slot_pipes(frames, 1, (("mesh", {"normals": "accumulate"}),
                                        ("mesh_clean", {"normals": "accumulate", "clean": 6})))
    out = {"frames_per_slot": frames, "unit": "ms per frame", "normals": "accumulate", "colors": True}
    out.update(alternate({name: fn(name) for name in pipes}, a.passes, frames))
    out["clean_adds_ms"] = round(out["mesh_clean"]["median_ms"] - out["mesh"]["median_ms"], 4)
    out["clean_stats_frame0"] = pipes["mesh_clean"].slots[0].mesh_buffers["clean_stats"][0].cpu().tolist()
    for p_ in pipes.values():
        p_.close()
    return out


SIMPLIFY_SETTINGS = (None, 128, 64)


def simplify(a, vol, netC, feat_C, calib, n=20):
    """reconstruct_mesh_many of n meshes at each simplify setting, with and without netC colours."""
    kwn = dict(netC=netC, feat_tensors_C=[feat_C] * n, calib_tensors=[calib] * n)
    ways, sizes = {}, {}
    for cells in SIMPLIFY_SETTINGS:
        ways["many_colours_%s" % cells] = (lambda cells=cells: reconstruct_mesh_many(
            [vol] * n, 0.5, BMIN, BMAX, simplify=cells, **kwn))
        ways["many_%s" % cells] = (lambda cells=cells: reconstruct_mesh_many([vol] * n, 0.5, BMIN, BMAX, simplify=cells))
        m = reconstruct_mesh(vol, 0.5, BMIN, BMAX, simplify=cells)
        sizes[str(cells)] = [int(m.verts.shape[0]), int(m.faces.shape[0])]
    out = {"resolutions": RES, "passes": a.passes, "per_pass": n, "unit": "ms per mesh", "normals": "accumulate",
           "vertices_faces": sizes}
    out.update(alternate(ways, a.passes, n))
    return out


def slot_simplify(a, frames=20):
    """The 20-frame colour slot with a mesh per frame at each simplify setting, per-frame ms of a submission
    (``meshes()`` included)."""
    pipes, fn = _slot_pipes(frames, 1, tuple(("mesh_%s" % cells, {"normals": "accumulate", "simplify": cells})
                                             for cells in SIMPLIFY_SETTINGS))
    out = {"frames_per_slot": frames, "unit": "ms per frame", "normals": "accumulate", "colors": True}
    out.update(alternate({name: fn(name) for name in pipes}, a.passes, frames))
    out["vertices_faces_frame0"] = {}
    for name, p_ in pipes.items():
        m = p_.slots[0].meshes()[0]
        out["vertices_faces_frame0"][name] = [int(m.verts.shape[0]), int(m.faces.shape[0])]
        p_.close()
    return out


def _glb_ref():
    """The numpy restatement of the file (tests/glb_ref.py): the host route's packing."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import glb_ref
    return glb_ref


def _host_glb(glb_ref, mesh):
    """The host route: every tensor of the ``Mesh`` to the host, packed by numpy."""
    return glb_ref.encode(mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), None, mesh.normals.cpu().numpy(),
                          mesh.colors.cpu().numpy(), b_min=BMIN, b_max=BMAX)


def glb_kernels(a, vol, netC, feat_C, calib, n=20):
    """mp_mesh_glb_batch over n coloured meshes (each its own buffers) at each simplify setting, a device copy of the
    same bytes, and the host route."""
    glb_ref = _glb_ref()
    out = {"resolutions": RES, "passes": a.passes, "per_pass": n, "unit": "ms per mesh", "launches_per_call": 3,
           "settings": {}}
    ways = {}
    for cells in SIMPLIFY_SETTINGS:
        m = reconstruct_mesh(vol, 0.5, BMIN, BMAX, netC=netC, feat_tensor_C=feat_C, calib_tensor=calib, simplify=cells)
        nv, nf = int(m.verts.shape[0]), int(m.faces.shape[0])
        size = ops.glb_bytes(nv, nf)
        moved = 36 * nv + 12 * nf + size  # f32 position, normal, colour and int32 corners in; the file out
        frames = [[t.clone() for t in (m.verts, m.faces, m.normals, m.colors)] for _ in range(n)]
        counts = torch.tensor([[nv, nf]] * n, dtype=torch.int32).to(DEV)
        files = torch.empty((n, size), dtype=torch.uint8, device=DEV)
        info = torch.empty((n, 2), dtype=torch.int32, device=DEV)
        src = torch.empty((n * moved // 2,), dtype=torch.uint8, device=DEV)
        dst = torch.empty_like(src)

        def encode(frames=frames, counts=counts, files=files, info=info):
            return ops.mesh_glb_raw_batch([f[0] for f in frames], [f[1] for f in frames], list(counts),
                                          [f[2] for f in frames], [f[3] for f in frames], "rows", 1.0, 0.0, BMIN, BMAX,
                                          out=files, info=info)
        encode()
        torch.cuda.synchronize()
        want = _host_glb(glb_ref, m)
        same = all(tuple(row) == (size, 0) for row in info.cpu().tolist()) and all(
            files[i].cpu().numpy().tobytes() == want for i in (0, n - 1))
        key = str(cells)
        out["settings"][key] = {"vertices": nv, "faces": nf, "file_bytes": size, "bytes_moved": moved,
                                "bytes_of_f32_tensors": 36 * nv + 12 * nf, "device_file_equals_host_packing": bool(same)}
        ways["glb_%s" % key] = encode
        ways["copy_%s" % key] = (lambda src=src, dst=dst: dst.copy_(src))
        ways["host_%s" % key] = (lambda m=m: [_host_glb(glb_ref, m) for _ in range(n)])
    out.update(alternate(ways, a.passes, n))
    for key, st in out["settings"].items():
        for way in ("glb", "copy"):
            st[way + "_gb_per_s"] = round(st["bytes_moved"] / (out["%s_%s" % (way, key)]["median_ms"] * 1e6), 1)
        st["glb_over_copy"] = round(out["glb_%s" % key]["median_ms"] / out["copy_%s" % key]["median_ms"], 3)
    return out


def slot_glb(a, frames=20):
    """The 20-frame colour slot with a mesh per frame: ``meshes()`` as the consumer, ``glbs()`` on a slot with
    ``encode_meshes``, and ``meshes()`` + ``.cpu()`` + the numpy packing; per-frame ms of a submission."""
    glb_ref = _glb_ref()
    mesh = {"normals": "accumulate"}
    pipes, fn = _slot_pipes(frames, 1, (("mesh", mesh), ("mesh_glb", mesh)), glbs={"mesh_glb": recon.Glb()})
    ways = {"meshes": fn("mesh"), "glbs": fn("mesh_glb", lambda s: s.glbs()),
            "meshes_cpu_numpy": fn("mesh", lambda s: [_host_glb(glb_ref, m) for m in s.meshes()])}
    out = {"frames_per_slot": frames, "unit": "ms per frame", "normals": "accumulate", "colors": True}
    out.update(alternate(ways, a.passes, frames))
    slot = pipes["mesh_glb"].slots[0]
    files, meshes = slot.glbs(), slot.meshes()
    out["file_bytes_frame0"] = len(files[0])
    out["vertices_faces_frame0"] = [int(meshes[0].verts.shape[0]), int(meshes[0].faces.shape[0])]
    out["capacity_bytes"] = int(slot.glb_bytes.shape[1])
    out["overflowed_frames"] = int(slot.glb_info[:, 1].sum().item())
    out["files_equal_host_packing"] = bool(all(f == _host_glb(glb_ref, m) for f, m in zip(files, meshes)))
    out["glbs_adds_ms"] = round(out["glbs"]["median_ms"] - out["meshes"]["median_ms"], 4)
    for p_ in pipes.values():
        p_.close()
    return out


TEXTURE_ATLASES = ((1024, 8), (2048, 16))


def _host_textured_glb(refs, slot, b, mesh, atlas):
    """The host route of a textured file: the mesh's tensors and netC's bake (on the slot's own maps) to the host, the
    image through Pillow's PNG encoder, the file through the numpy restatement's writer."""
    import io
    from PIL import Image
    glb_ref, tex_ref = refs
    nchw = slot.feats_hwc_c[b].permute(2, 0, 1)[None].contiguous()
    image, _ = recon.bake_texture(mesh, atlas, netC=slot.netC, feat_tensors_C=[[nchw]], calib_tensors=slot.calib[b:b + 1])
    png = io.BytesIO()
    Image.fromarray(glb_ref.to_u8(image.cpu().numpy()).astype(np.uint8)).save(png, format="PNG")
    return tex_ref.encode(mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), atlas.size, atlas.cell, png.getvalue(), None,
                          mesh.normals.cpu().numpy(), BMIN, BMAX)[0]


def slot_texture(a, frames=20, simplify=64):
    """The 20-frame colour slot with a simplified mesh per frame, ``glbs()`` as the consumer: COLOR_0 against a baked
    atlas of two sizes, and the textured file through the host; per-frame ms of a submission."""
    glb_ref = _glb_ref()
    import glb_texture_ref as tex_ref
    coloured = {"normals": "accumulate", "simplify": simplify}
    bare = dict(coloured, colors=False)
    atlases = {"atlas_%d_%d" % st: recon.Atlas(*st) for st in TEXTURE_ATLASES}
    glbs = dict({"color_0": recon.Glb()}, **{k: recon.Glb(texture=t) for k, t in atlases.items()})
    pipes, fn = _slot_pipes(frames, 1, (("color_0", coloured), ("bare", bare)) + tuple((k, bare) for k in atlases), glbs=glbs)
    first = next(iter(atlases))
    ways = {name: fn(name, lambda s: s.glbs()) for name in glbs}
    ways["host_" + first] = fn("bare", lambda s: [_host_textured_glb((glb_ref, tex_ref), s, b, m, atlases[first])
                                                  for b, m in enumerate(s.meshes())])
    out = {"frames_per_slot": frames, "unit": "ms per frame", "normals": "accumulate", "simplify": simplify,
           "resolutions": RES}
    out.update(alternate(ways, a.passes, frames))
    for name in glbs:
        slot = pipes[name].slots[0]
        files, meshes = slot.glbs(), slot.meshes()
        st = {"file_bytes_frame0": len(files[0]), "capacity_bytes": int(slot.glb_bytes.shape[1]),
              "vertices_faces_frame0": [int(meshes[0].verts.shape[0]), int(meshes[0].faces.shape[0])],
              "frames_encoded_again": int((slot.glb_info[:, 1] != 0).sum().item())}
        if name in atlases:
            counts = slot.atlas_lists["count"][:, 1].cpu().tolist()
            st.update(atlas_faces=atlases[name].faces, texels_queried_per_frame=int(np.mean(counts)),
                      texels_queried_frame0=int(counts[0]), png_bytes_frame0=int(slot.atlas_png_info[0, 0].item()),
                      png_capacity=int(slot.atlas_png.shape[1]),
                      adds_ms_over_color_0=round(out[name]["median_ms"] - out["color_0"]["median_ms"], 4))
            got = tex_ref.read(files[0])
            st["image_decodes_to_the_bake"] = bool(np.array_equal(
                tex_ref.decode_png(got["png"]), glb_ref.to_u8(slot.atlas_image[0].cpu().numpy())))
        out[name + "_file"] = st
    for p_ in pipes.values():
        p_.close()
    return out


SMOOTH_SETTINGS = (None, 2, 10)


def smooth(a, vol, netC, feat_C, calib, n=20):
    """reconstruct_mesh_many of n meshes at each smooth setting: without colours, with netC colours, and with colours
    behind simplify=128."""
    kwn = dict(netC=netC, feat_tensors_C=[feat_C] * n, calib_tensors=[calib] * n)
    ways, sizes = {}, {}
    for it in SMOOTH_SETTINGS:
        ways["many_%s" % it] = (lambda it=it: reconstruct_mesh_many([vol] * n, 0.5, BMIN, BMAX, smooth=it))
        ways["many_colours_%s" % it] = (lambda it=it: reconstruct_mesh_many([vol] * n, 0.5, BMIN, BMAX, smooth=it, **kwn))
        ways["many_colours_simplify128_%s" % it] = (lambda it=it: reconstruct_mesh_many(
            [vol] * n, 0.5, BMIN, BMAX, simplify=128, smooth=it, **kwn))
    for cells in (None, 128):
        m = reconstruct_mesh(vol, 0.5, BMIN, BMAX, simplify=cells, smooth=2)
        sizes["simplify_%s" % cells] = [int(m.verts.shape[0]), int(m.faces.shape[0])]
    out = {"resolutions": RES, "passes": a.passes, "per_pass": n, "unit": "ms per mesh", "normals": "accumulate",
           "lam_mu": [0.5, -0.53], "vertices_faces": sizes,
           "launches_per_smoothing_call": {str(it): {"kernels": 4 + 2 * it, "memsets": 1} for it in SMOOTH_SETTINGS if it}}
    out.update(alternate(ways, a.passes, n))
    for kind in ("many", "many_colours", "many_colours_simplify128"):
        for it in SMOOTH_SETTINGS[1:]:
            out["%s_smooth_%d_adds_ms" % (kind, it)] = round(
                out["%s_%d" % (kind, it)]["median_ms"] - out["%s_None" % kind]["median_ms"], 4)
    return out


def slot_deferred(a, frames=20):
    """The 20-frame colour slot with pictures: today's per-vertex colours against netC at the covered pixels, per-frame ms
    of a submission (``pictures()`` included), and what each picture covers."""
    cams = torch.cat([recon.pifu_calib(*syn.scene_camera(30 * k + 15), device="cpu") for k in range(4)])
    mesh_c, mesh_n = {"normals": "accumulate", "colors": True}, {"normals": "accumulate", "colors": False}
    rows = (("vertex_colours_257_views1", mesh_c, dict(views=1, res=257, shade="colors"), cams[:1]),
            ("netC_257_views1", mesh_n, dict(views=1, res=257, shade="netC"), cams[:1]),
            ("netC_257_views4", mesh_n, dict(views=4, res=257, shade="netC"), cams),
            ("netC_1024_views1", mesh_n, dict(views=1, res=1024, shade="netC"), cams[:1]))
    pipes, fn = _slot_pipes(frames, 1, rows)
    out = {"frames_per_slot": frames, "unit": "ms per frame", "normals": "accumulate",
           "cameras": "scene_camera(15 + 30 k): turned off the axes"}
    out.update(alternate({name: fn(name) for name in pipes}, a.passes, frames))
    out["covered_pixels_per_picture_frame0"], out["vertices_frame0"] = {}, {}
    for name, p_ in pipes.items():
        slot = p_.slots[0]
        pic, m = slot.pictures()[0], slot.meshes()[0]
        out["covered_pixels_per_picture_frame0"][name] = [int((f >= 0).sum().item()) for f in pic.face]
        out["vertices_frame0"][name] = int(m.verts.shape[0])
        p_.close()
    base = out["vertex_colours_257_views1"]["median_ms"]
    out["netC_257_views1_minus_vertex_colours_ms"] = round(out["netC_257_views1"]["median_ms"] - base, 4)
    return out


def _scene_setup(light=None):
    """The floor, the camera, the mesh options and the picture options that --scene and --shadow share."""
    i, j = np.meshgrid(np.arange(2048), np.arange(2048), indexing="ij")
    tex = np.stack([(((i // 64) + (j // 64)) % 2) * 200 + 40, i // 8, j // 8], -1).astype(np.uint8)
    y = -0.9
    floor = recon.Scene([[-1.5, y, -1.5], [1.5, y, -1.5], [1.5, y, 1.5], [-1.5, y, 1.5]], [[0, 1, 2], [0, 2, 3]],
                        [[0, 0], [1, 0], [1, 1], [0, 1]], tex, device=DEV, light=light)
    c, s_ = np.cos(-0.35), np.sin(-0.35)  # from above: the floor fills the lower part
    cam = np.eye(4, dtype=np.float32)
    cam[:3, :3] = np.diag([2.0, 2.0, 1.0]) @ np.array([[1, 0, 0], [0, c, -s_], [0, s_, c]])
    cam[:3, 3] = [0.0, 0.0, 2.6]
    cam = torch.from_numpy(cam)[None]
    mesh = {"normals": "accumulate", "colors": False}
    base = dict(views=1, shade="normals", projection="perspective", nearest="min", near=0.3, perspective_correct=True)
    return floor, cam, mesh, base


def slot_shadow(a, frames=20):
    """The --scene slots with the floor, without and with a directional light on it (a 512^2 shadow map, radius 1):
    per-frame ms of a submission (``pictures()`` included) at one 257^2 and one 1024^2 view, and the pixels of frame 0
    that the shadow darkens."""
    sun = recon.Light.directional((0.4, -1.0, 0.3), (-1.5, -0.9, -1.5), (1.5, 1.0, 1.5), res=512, radius=1)
    floor, cam, mesh, base = _scene_setup()
    lit = _scene_setup(sun)[0]
    rows = (("scene_257", mesh, dict(base, res=257, scene=floor), cam), ("lit_257", mesh, dict(base, res=257, scene=lit), cam),
            ("scene_1024", mesh, dict(base, res=1024, scene=floor), cam),
            ("lit_1024", mesh, dict(base, res=1024, scene=lit), cam))
    pipes, fn = _slot_pipes(frames, 1, rows)
    out = {"frames_per_slot": frames, "unit": "ms per frame", "shadow_map": list(sun.res), "radius": sun.radius,
           "light": "directional (0.4, -1, 0.3), fitted to the box of the floor and the body",
           "camera": "perspective, turned -0.35 rad about x (looking down), near 0.3, perspective-correct"}
    out.update(alternate({name: fn(name) for name in pipes}, a.passes, frames))
    out["shadowed_pixels_frame0"] = {}
    for name, p_ in pipes.items():
        slot = p_.slots[0]
        slot.pictures()
        if hasattr(slot, "scene_lit"):
            out["shadowed_pixels_frame0"][name] = int((slot.scene_lit[0] != slot.scene_image[0]).any(-1).sum().item())
        p_.close()
    for res in ("257", "1024"):
        lit_row, plain = out["lit_" + res], out["scene_" + res]
        out["lit_%s_minus_scene_ms" % res] = round(lit_row["median_ms"] - plain["median_ms"], 4)
        out["lit_%s_inside_the_spread" % res] = bool(
            lit_row["median_ms"] - plain["median_ms"] <= max(lit_row["max_ms"] - lit_row["min_ms"],
                                                             plain["max_ms"] - plain["min_ms"]))
    return out


def slot_lighting(a, frames=20):
    """The --shadow slots with the light on the scene, without and with ``lighting=`` on the subject (clay, SH in the
    camera's frame, a direct term along the sun, the self-shadow): per-frame ms of a submission (``pictures()``
    included) at one 257^2 and one 1024^2 view, and the pixels of frame 0 that the lighting changes."""
    direction = (0.4, -1.0, 0.3)
    sun = recon.Light.directional(direction, (-1.5, -0.9, -1.5), (1.5, 1.0, 1.5), res=512, radius=1)
    floor, cam, mesh, base = _scene_setup(sun)
    sh = np.random.RandomState(0).uniform(-0.2, 0.4, (9, 3)).astype(np.float32)
    sh[0] += 0.8
    lighting = recon.Lighting(sh, direct=(direction, (0.9, 0.85, 0.8)), frame="camera", albedo=(0.8, 0.7, 0.6),
                              self_shadow=0.02)
    rows = []
    for res in (257, 1024):
        rows.append(("shadow_%d" % res, mesh, dict(base, res=res, scene=floor), cam))
        rows.append(("lighting_%d" % res, mesh, dict(base, res=res, scene=floor), cam, dict(lighting=lighting)))
    pipes, fn = _slot_pipes(frames, 1, rows)
    out = {"frames_per_slot": frames, "unit": "ms per frame", "shadow_map": list(sun.res), "radius": sun.radius,
           "light": "directional (0.4, -1, 0.3), fitted to the box of the floor and the body",
           "lighting": "clay albedo, 9 x 3 SH coefficients in the camera's frame, a direct term along the light, "
                       "self_shadow 0.02, gamma 1",
           "camera": "perspective, turned -0.35 rad about x (looking down), near 0.3, perspective-correct"}
    out.update(alternate({name: fn(name) for name in pipes}, a.passes, frames))
    pictures = {}
    for name, p_ in pipes.items():
        pictures[name] = p_.slots[0].pictures()[0].image.clone()
        p_.close()
    out["lit_pixels_frame0"] = {}
    for res in ("257", "1024"):
        lit_row, plain = out["lighting_" + res], out["shadow_" + res]
        out["lit_pixels_frame0"][res] = int((pictures["lighting_" + res] != pictures["shadow_" + res]).any(-1).sum().item())
        out["lighting_%s_minus_shadow_ms" % res] = round(lit_row["median_ms"] - plain["median_ms"], 4)
        out["lighting_%s_inside_the_spread" % res] = bool(
            lit_row["median_ms"] - plain["median_ms"] <= max(lit_row["max_ms"] - lit_row["min_ms"],
                                                             plain["max_ms"] - plain["min_ms"]))
    return out


def slot_jpeg(a, frames=20):
    """mp_picture_jpeg alone on a batch of ``frames`` lit pictures (ms per picture, bytes per file) at 257^2 and 1024^2,
    quality 90, 420 and 444; then the --lighting slots without and with ``encode_pictures``, with ``pictures()`` against
    ``jpegs()`` as the consumer (ms per frame of a submission); and, where Pillow is importable, the only way to a JPEG
    without the feature: ``pictures()``, ``.cpu()``, Pillow ``save`` on the host."""
    import io
    try:
        from PIL import Image
    except ImportError:
        Image = None
    direction = (0.4, -1.0, 0.3)
    sun = recon.Light.directional(direction, (-1.5, -0.9, -1.5), (1.5, 1.0, 1.5), res=512, radius=1)
    floor, cam, mesh, base = _scene_setup(sun)
    sh = np.random.RandomState(0).uniform(-0.2, 0.4, (9, 3)).astype(np.float32)
    sh[0] += 0.8
    lighting = recon.Lighting(sh, direct=(direction, (0.9, 0.85, 0.8)), frame="camera", albedo=(0.8, 0.7, 0.6),
                              self_shadow=0.02)
    jpeg = recon.Jpeg(quality=90, subsampling="420")
    rows = []
    for res in (257, 1024):
        opts = dict(base, res=res, scene=floor)
        rows.append(("pictures_%d" % res, mesh, opts, cam, dict(lighting=lighting)))
        rows.append(("encode_%d" % res, mesh, opts, cam, dict(lighting=lighting, encode_pictures=jpeg)))
    pipes, fn = _slot_pipes(frames, 1, rows)

    def on_host(s):
        files = []
        for pic in s.pictures():
            u8 = (pic.image.clamp(0, 1) * 255 + 0.5).to(torch.uint8).cpu().numpy()
            for v in range(u8.shape[0]):
                buf = io.BytesIO()
                Image.fromarray(u8[v]).save(buf, "JPEG", quality=90, subsampling=2)
                files.append(buf.getvalue())
        return files

    ways = {}
    for res in (257, 1024):
        ways["pictures_%d" % res] = fn("pictures_%d" % res)
        ways["encode_%d_pictures" % res] = fn("encode_%d" % res)
        ways["encode_%d_jpegs" % res] = fn("encode_%d" % res, lambda s: s.jpegs())
        if Image is not None:
            ways["host_pillow_%d" % res] = fn("pictures_%d" % res, on_host)
    out = {"frames_per_slot": frames, "unit": "ms per frame", "quality": 90, "pillow": Image is not None,
           "slots": "the --lighting slots: one view, the floor with its light, clay lighting with the self-shadow",
           "consumers": "pictures(): views of the device buffers; jpegs(): the files as bytes on the host; host_pillow: "
                        "pictures(), 8 bit on the device, .cpu(), Pillow save at quality 90, 420"}
    out.update(alternate(ways, a.passes, frames))
    # the kernels alone, on the pictures the slots made
    kernels = {}
    out["file_bytes"] = {}
    for res in (257, 1024):
        slot = pipes["encode_%d" % res].slots[0]
        files = slot.jpegs()
        out["file_bytes"]["%d_420_slot" % res] = stats([len(f[0]) for f in files])["median_ms"]
        images = slot.pictures_image[:frames].reshape(frames, res, res, 3).clone()
        for sub in ("420", "444"):
            cap = recon.Jpeg(subsampling=sub).capacity_for(res, res)
            bufs = (torch.empty((frames, cap), dtype=torch.uint8, device=DEV),
                    torch.empty((frames, 2), dtype=torch.int32, device=DEV))
            kernels["mp_picture_jpeg_%d_%s" % (res, sub)] = (
                lambda images=images, sub=sub, bufs=bufs: ops.picture_jpeg_raw(images, 90, sub, None, out=bufs[0],
                                                                               info=bufs[1]))
            info = kernels["mp_picture_jpeg_%d_%s" % (res, sub)]()[1].cpu().numpy()
            assert not info[:, 1].any()
            out["file_bytes"]["%d_%s" % (res, sub)] = float(np.median(info[:, 0]))
    for p_ in pipes.values():
        p_.close()
    out["kernels_unit"] = "ms per picture, a batch of %d" % frames
    out["kernels"] = alternate(kernels, a.passes, frames)
    for res in ("257", "1024"):
        out["encode_%s_jpegs_minus_pictures_ms" % res] = round(
            out["encode_%s_jpegs" % res]["median_ms"] - out["pictures_" + res]["median_ms"], 4)
    return out


def slot_png(a, frames=20):
    """mp_picture_png alone on a batch of ``frames`` lit pictures (ms per picture, bytes per file) at 257^2 and 1024^2
    for RGB8, RGBA8 (alpha: the subject's mask) and GRAY16 (the depth over 0..6); then the --lighting slots without and
    with a ``recon.Png``, with ``pictures()`` against ``pngs()`` as the consumer (ms per frame of a submission), and the
    way to a PNG without the feature: ``pictures()``, ``.cpu()``, Pillow ``save(compress_level=6)`` on the host."""
    import io
    from PIL import Image
    direction = (0.4, -1.0, 0.3)
    sun = recon.Light.directional(direction, (-1.5, -0.9, -1.5), (1.5, 1.0, 1.5), res=512, radius=1)
    floor, cam, mesh, base = _scene_setup(sun)
    sh = np.random.RandomState(0).uniform(-0.2, 0.4, (9, 3)).astype(np.float32)
    sh[0] += 0.8
    lighting = recon.Lighting(sh, direct=(direction, (0.9, 0.85, 0.8)), frame="camera", albedo=(0.8, 0.7, 0.6),
                              self_shadow=0.02)
    png = recon.Png()
    rows = []
    for res in (257, 1024):
        opts = dict(base, res=res, scene=floor)
        rows.append(("pictures_%d" % res, mesh, opts, cam, dict(lighting=lighting)))
        rows.append(("encode_%d" % res, mesh, opts, cam, dict(lighting=lighting, encode_pictures=png)))
    pipes, fn = _slot_pipes(frames, 1, rows)

    def on_host(s):
        files = []
        for pic in s.pictures():
            u8 = (pic.image.clamp(0, 1) * 255 + 0.5).to(torch.uint8).cpu().numpy()
            for v in range(u8.shape[0]):
                buf = io.BytesIO()
                Image.fromarray(u8[v]).save(buf, "PNG", compress_level=6)
                files.append(buf.getvalue())
        return files

    ways = {}
    for res in (257, 1024):
        ways["pictures_%d" % res] = fn("pictures_%d" % res)
        ways["encode_%d_pictures" % res] = fn("encode_%d" % res)
        ways["encode_%d_pngs" % res] = fn("encode_%d" % res, lambda s: s.pngs())
        ways["host_pillow_%d" % res] = fn("pictures_%d" % res, on_host)
    out = {"frames_per_slot": frames, "unit": "ms per frame", "filter": "adaptive",
           "slots": "the --lighting slots: one view, the floor with its light, clay lighting with the self-shadow",
           "consumers": "pictures(): views of the device buffers; pngs(): the files as bytes on the host; host_pillow: "
                        "pictures(), 8 bit on the device, .cpu(), Pillow save at compress_level 6"}
    out.update(alternate(ways, a.passes, frames))
    kernels = {}
    out["file_bytes"] = {}
    for res in (257, 1024):
        slot = pipes["encode_%d" % res].slots[0]
        out["file_bytes"]["%d_rgb8_slot" % res] = stats([len(f[0]) for f in slot.pngs()])["median_ms"]
        out["file_bytes"]["%d_rgb8_pillow" % res] = float(np.median([len(f) for f in on_host(slot)]))
        planes = {"rgb8": (slot.pictures_image[:frames].reshape(frames, res, res, 3).clone(), None),
                  "gray16": (slot.pictures_depth[:frames].reshape(frames, res, res).clone(), None)}
        planes["rgba8"] = (planes["rgb8"][0], (slot.pictures_mask[:frames].reshape(frames, res, res) == 2).float())
        for fmt, (images, alpha) in planes.items():
            cap = 4096 + res * res * {"rgb8": 3, "rgba8": 4, "gray16": 2}[fmt] // 2
            bufs = (torch.empty((frames, cap), dtype=torch.uint8, device=DEV),
                    torch.empty((frames, 2), dtype=torch.int32, device=DEV))
            name = "mp_picture_png_%d_%s" % (res, fmt)
            kernels[name] = (lambda images=images, alpha=alpha, fmt=fmt, bufs=bufs: ops.picture_png_raw(
                images, alpha, fmt, "adaptive", 0.0, 1.0 / 6.0, out=bufs[0], info=bufs[1]))
            info = kernels[name]()[1].cpu().numpy()
            assert not info[:, 1].any()
            out["file_bytes"]["%d_%s" % (res, fmt)] = float(np.median(info[:, 0]))
    for p_ in pipes.values():
        p_.close()
    out["kernels_unit"] = "ms per picture, a batch of %d" % frames
    out["kernels"] = alternate(kernels, a.passes, frames)
    for res in ("257", "1024"):
        out["encode_%s_pngs_minus_pictures_ms" % res] = round(
            out["encode_%s_pngs" % res]["median_ms"] - out["pictures_" + res]["median_ms"], 4)
        out["pngs_over_host_pillow_%s" % res] = round(
            out["encode_%s_pngs" % res]["median_ms"] / out["host_pillow_" + res]["median_ms"], 4)
    return out


def resolve_kernels(a, n=20):
    """mp_picture_resolve_batch alone on a batch of ``n`` pictures with every plane given and wanted, per picture, at
    the final sizes 257^2 and 1024^2 for samples 2 and 4, beside a device-to-device copy that moves the same number of
    bytes (read plus written) -- all in the same alternating passes."""
    out = {"pictures_per_call": n, "unit": "ms per picture", "planes": "image, depth, face ids, mask in; image, depth, "
           "face ids, mask, coverage out", "bytes": "read plus written, per picture"}
    ways, traffic, keep, ctx = {}, {}, [], ops.get_context(torch.device(DEV))
    for res in (257, 1024):
        for s in (2, 4):
            fine = (n, 1, s * res, s * res)
            ins = ([t for t in torch.rand(fine + (3,), device=DEV)], [t for t in torch.rand(fine, device=DEV)],
                   [t for t in torch.randint(-1, 1000, fine, dtype=torch.int32, device=DEV)],
                   [t for t in torch.randint(0, 3, fine, dtype=torch.uint8, device=DEV)])
            small = (n, 1, res, res)
            outs = (torch.empty(small + (3,), device=DEV), torch.empty(small, device=DEV),
                    torch.empty(small, dtype=torch.int32, device=DEV), torch.empty(small, dtype=torch.uint8, device=DEV),
                    torch.empty(small, device=DEV))
            name = "resolve_%d_s%d" % (res, s)
            traffic[name] = 21 * (s * res) ** 2 + 25 * res ** 2
            args = ([ops._ptr_array(p) for p in ins] + [res, res, s, ops.NEAREST_MODES["min"]]
                    + [ops._ptr_array(list(o)) for o in outs] + [ops._stream(outs[0])])
            keep.append((ins, outs))
            # the entry point itself, on pointer arrays made once; the wrapper's checks cost the host ~0.5 ms a call
            ways[name] = lambda args=args: ctx.check(ctx.lib.mp_picture_resolve_batch(ctx.handle, n, 1, *args), name)
            if (res, s) == (257, 2):
                ways["wrapper_257_s2"] = lambda ins=ins, outs=outs: ops.picture_resolve_batch(*ins, 2, "min", out=outs)
                traffic["wrapper_257_s2"] = traffic[name]
            src = torch.empty(n * traffic[name] // 2, dtype=torch.uint8, device=DEV)
            dst = torch.empty_like(src)
            traffic["copy_%d_s%d" % (res, s)] = 2 * (traffic[name] // 2)
            ways["copy_%d_s%d" % (res, s)] = lambda src=src, dst=dst: dst.copy_(src)
    out.update(alternate(ways, a.passes, n))  # wall clock of ONE call and a sync: the host side of the call included
    # the device alone: events around calls enqueued back to back (200 at 257^2, 20 at 1024^2), in alternating passes
    device = {name: [] for name in ways}
    for _ in range(a.passes):
        for name, fn in ways.items():
            reps = 200 if "_257_" in name else 20
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _k in range(reps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            device[name].append(t0.elapsed_time(t1) / reps / n)
    out["device"] = {name: stats(t) for name, t in device.items()}
    out["device_unit"] = ("ms per picture between two events around calls enqueued back to back: 200 at 257^2, 20 at "
                          "1024^2")
    out["bytes_per_picture"] = traffic
    out["gb_per_s"] = {name: round(traffic[name] / (out["device"][name]["median_ms"] * 1e-3) / 1e9, 1) for name in ways}
    out["gb_per_s_wall_clock_of_one_call"] = {name: round(traffic[name] / (out[name]["median_ms"] * 1e-3) / 1e9, 1)
                                              for name in ways}
    out["resolve_over_copy_rate"] = {k[8:]: round(out["gb_per_s"][k] / out["gb_per_s"]["copy_" + k[8:]], 3)
                                     for k in ways if k.startswith("resolve_")}
    return out


def slot_samples(a, frames=20):
    """The --jpeg slots WITH ``encode_pictures`` -- one view, the floor with its light, clay lighting with the
    self-shadow, ``jpegs()`` as the consumer -- at ``samples`` absent / 2 / 4 for 257^2 and absent / 2 for 1024^2:
    per-frame ms of a submission, and the pixels of frame 0 whose coverage is strictly between 0 and 1."""
    direction = (0.4, -1.0, 0.3)
    sun = recon.Light.directional(direction, (-1.5, -0.9, -1.5), (1.5, 1.0, 1.5), res=512, radius=1)
    floor, cam, mesh, base = _scene_setup(sun)
    sh = np.random.RandomState(0).uniform(-0.2, 0.4, (9, 3)).astype(np.float32)
    sh[0] += 0.8
    lighting = recon.Lighting(sh, direct=(direction, (0.9, 0.85, 0.8)), frame="camera", albedo=(0.8, 0.7, 0.6),
                              self_shadow=0.02)
    more = dict(lighting=lighting, encode_pictures=recon.Jpeg(quality=90, subsampling="420"))
    out = {"frames_per_slot": frames, "unit": "ms per frame", "consumer": "jpegs()",
           "slots": "the --jpeg slots: one view, the floor with its light, clay lighting with the self-shadow, "
                    "encode_pictures at quality 90, 420"}
    out["edge_pixels_frame0"] = {}
    for res, counts in ((257, (1, 2, 4)), (1024, (1, 2))):  # one size at a time: the working buffers are large
        rows = [("samples%d_%d" % (s, res), mesh, dict(base, res=res, scene=floor, **({} if s == 1 else {"samples": s})),
                 cam, more) for s in counts]
        pipes, fn = _slot_pipes(frames, 1, rows)
        out.update(alternate({name: fn(name, lambda s_: s_.jpegs()) for name in pipes}, a.passes, frames))
        for name, p_ in pipes.items():
            cov = p_.slots[0].pictures_coverage
            if cov is not None:
                out["edge_pixels_frame0"][name] = int(((cov[0] > 0) & (cov[0] < 1)).sum().item())
            p_.close()
        del pipes, fn
        torch.cuda.empty_cache()
        for s in counts[1:]:
            out["samples%d_%d_minus_samples1_ms" % (s, res)] = round(
                out["samples%d_%d" % (s, res)]["median_ms"] - out["samples1_%d" % res]["median_ms"], 4)
    return out


def _definition_samples(verts, normals, occ, blocks, t, r, rays):
    """The samples mp_mesh_transfer's definition visits on one mesh, and those of them in an empty 8^3 block: the same
    f32 expressions in torch, every sample of every ray (no skipping), a chunk of vertices at a time."""
    bias_w, step_w, steps = rays
    dirs = torch.from_numpy(t.dirs).to(DEV)
    f = torch.float32
    lo, hi = torch.tensor(BMIN, dtype=f, device=DEV), torch.tensor(BMAX, dtype=f, device=DEV)
    vox = r / (hi - lo)
    s2 = (normals * normals).sum(1, keepdim=True)
    u = torch.where(torch.isfinite(s2) & (s2 > 0), normals / s2.sqrt(), torch.zeros_like(normals))
    o = ((verts - lo) / (hi - lo)) * r + (bias_w * u) * vox
    delta = (step_w * dirs) * vox
    visited = empty = 0
    for v0 in range(0, verts.shape[0], 16384):
        oc, uc = o[v0:v0 + 16384], u[v0:v0 + 16384]
        vi, di = torch.nonzero((uc @ dirs.t()) > 0, as_tuple=True)
        for j in range(steps):
            if vi.numel() == 0:
                break
            s = oc[vi] + float(j) * delta[di]
            inside = ((s >= 0) & (s < r)).all(1)
            vi, di, s = vi[inside], di[inside], s[inside]
            visited += int(inside.numel())
            c = s.floor().long()
            empty += int((~blocks[c[:, 2] >> 3, c[:, 1] >> 3, c[:, 0] >> 3]).sum().item())
            hit = occ[c[:, 2], c[:, 1], c[:, 0]]
            vi, di = vi[~hit], di[~hit]
    return visited, empty


def transfer_kernels(a, n=20):
    """Per mesh in a batch of ``n`` on the 257^3 body: mp_volume_bits, mp_mesh_transfer and mp_mesh_transfer_shade each
    alone, at D = 64, 128 and 256."""
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    fh = ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2))[None].to(DEV))
    cal = torch.from_numpy(orc.pifu_calib(*syn.scene_camera(30))).to(DEV)
    vol, status = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES)
    assert int(status[0].item()) == 1
    r = int(vol.shape[-1])
    mesh = reconstruct_mesh(vol[None, None], 0.5, BMIN, BMAX, normals="accumulate")
    nv = int(mesh.verts.shape[0])
    vols = [vol.clone() for _ in range(n)]
    verts, normals = [mesh.verts.contiguous().clone() for _ in range(n)], [mesh.normals.contiguous().clone() for _ in range(n)]
    counts = [torch.tensor([nv, int(mesh.faces.shape[0])], dtype=torch.int32, device=DEV) for _ in range(n)]
    bits = torch.empty((n, ops.volume_bits_words(r)), dtype=torch.int32, device=DEV)
    prt = torch.empty((n, nv, 9), dtype=torch.float32, device=DEV)
    shade = torch.empty((n, nv, 3), dtype=torch.float32, device=DEV)
    sh = np.random.RandomState(0).uniform(-0.2, 0.4, (9, 3)).astype(np.float32)
    occ = vol.reshape(r, r, r) > 0.5
    nb = (r + 7) // 8
    padded = torch.zeros((nb * 8,) * 3, dtype=torch.bool, device=DEV)
    padded[:r, :r, :r] = occ
    blocks = padded.reshape(nb, 8, nb, 8, nb, 8).any(5).any(3).any(1)
    out = {"resolution": r, "vertices": nv, "meshes_per_call": n, "unit": "ms per mesh", "passes": a.passes,
           "bias": 1.5, "step": 1.0, "bits_kib_per_frame": round(bits.shape[1] * 4 / 1024, 1),
           "occupied_blocks_share": round(float(blocks.float().mean().item()), 4),
           "one_more_reconstruction_ms": 5.75}
    ways = {"bits": lambda: ops.volume_bits_raw_batch(vols, 0.5, out=bits)}
    tables = {}
    for d in (64, 128, 256):
        t = recon.Transfer(d)
        rays = t.rays(r, BMIN, BMAX)
        tables[d] = (t, rays)
        dirs, basis = t.tables(DEV)

        def trace(dirs=dirs, basis=basis, t=t, rays=rays):
            ops.mesh_transfer_raw_batch(verts, normals, counts, list(bits), r, BMIN, BMAX, dirs, basis, t.weight, *rays,
                                        want=(False, True), out=(None, prt))
        ways["transfer_%d" % d] = trace
    ways["shade"] = lambda: ops.mesh_transfer_shade_raw_batch(list(prt), counts, sh, out=shade)
    out.update(alternate(ways, a.passes, n))
    for d, (t, rays) in tables.items():
        visited, empty = _definition_samples(verts[0], normals[0], occ, blocks, t, r, rays)
        row = out["transfer_%d" % d]
        row["max_steps"] = rays[2]
        row["definition_samples_per_mesh"] = visited
        row["definition_samples_per_s"] = round(visited / (row["median_ms"] * 1e-3))
        row["samples_in_empty_blocks_share"] = round(empty / max(visited, 1), 4)
        row["costs_more_than_one_reconstruction"] = bool(row["median_ms"] > out["one_more_reconstruction_ms"])
    return out


def slot_transfer(a, frames=20):
    """The --lighting slots (clay, SH in the world frame, a direct term, no self-shadow) without and with ``transfer=``:
    per-frame ms of a submission (``pictures()`` included) at one 257^2 and one 1024^2 view."""
    direction = (0.4, -1.0, 0.3)
    sun = recon.Light.directional(direction, (-1.5, -0.9, -1.5), (1.5, 1.0, 1.5), res=512, radius=1)
    floor, cam, mesh, base = _scene_setup(sun)
    sh = np.random.RandomState(0).uniform(-0.2, 0.4, (9, 3)).astype(np.float32)
    sh[0] += 0.8
    kw = dict(direct=(direction, (0.9, 0.85, 0.8)), albedo=(0.8, 0.7, 0.6))
    rows = []
    for res in (257, 1024):
        rows.append(("lighting_%d" % res, mesh, dict(base, res=res, scene=floor), cam,
                     dict(lighting=recon.Lighting(sh, **kw))))
        rows.append(("transfer_%d" % res, mesh, dict(base, res=res, scene=floor), cam,
                     dict(lighting=recon.Lighting(sh, transfer=recon.Transfer(128), **kw))))
    pipes, fn = _slot_pipes(frames, 1, rows)
    out = {"frames_per_slot": frames, "unit": "ms per frame", "directions": 128, "bias": 1.5, "step": 1.0,
           "lighting": "clay albedo, 9 x 3 SH coefficients in the world frame, a direct term along the light, gamma 1",
           "camera": "perspective, turned -0.35 rad about x (looking down), near 0.3, perspective-correct"}
    out.update(alternate({name: fn(name) for name in pipes}, a.passes, frames))
    pictures = {}
    for name, p_ in pipes.items():
        pictures[name] = p_.slots[0].pictures()[0].image.clone()
        p_.close()
    out["changed_pixels_frame0"] = {}
    for res in ("257", "1024"):
        with_t, plain = out["transfer_" + res], out["lighting_" + res]
        out["changed_pixels_frame0"][res] = int((pictures["transfer_" + res] != pictures["lighting_" + res]).any(-1).sum().item())
        out["transfer_%s_minus_lighting_ms" % res] = round(with_t["median_ms"] - plain["median_ms"], 4)
        out["transfer_%s_spread_ms" % res] = round(max(with_t["max_ms"] - with_t["min_ms"],
                                                       plain["max_ms"] - plain["min_ms"]), 4)
    return out


def slot_scene(a, frames=20):
    """The 20-frame slot with normal-shaded pictures under a free perspective camera, with and without a textured 3 m
    floor (a 2048^2 checker, full mip chain) composited behind the subject by depth: per-frame ms of a submission
    (``pictures()`` included) at one 257^2 and one 1024^2 view, and what the composite shows in frame 0."""
    floor, cam, mesh, base = _scene_setup()
    rows = (("plain_257", mesh, dict(base, res=257), cam), ("scene_257", mesh, dict(base, res=257, scene=floor), cam),
            ("plain_1024", mesh, dict(base, res=1024), cam), ("scene_1024", mesh, dict(base, res=1024, scene=floor), cam))
    pipes, fn = _slot_pipes(frames, 1, rows)
    out = {"frames_per_slot": frames, "unit": "ms per frame", "texture": [2048, 2048], "levels": floor.levels,
           "camera": "perspective, turned -0.35 rad about x (looking down), near 0.3, perspective-correct"}
    out.update(alternate({name: fn(name) for name in pipes}, a.passes, frames))
    out["mask_counts_frame0"] = {}
    for name, p_ in pipes.items():
        pic = p_.slots[0].pictures()[0]
        if hasattr(pic, "mask"):
            out["mask_counts_frame0"][name] = torch.bincount(pic.mask.reshape(-1).long(), minlength=3).tolist()
        p_.close()
    for res in ("257", "1024"):
        out["scene_%s_minus_plain_ms" % res] = round(out["scene_" + res]["median_ms"] - out["plain_" + res]["median_ms"], 4)
    return out


def _slot_pipes(frames, depth, meshes, glbs=None):
    """FramePipelines of the bench's synthetic frames, one per (name, mesh option[, pictures option, cameras]), and
    fn(name) -> a submission.  ``glbs``: None, or {name: the ``recon.Glb`` of that pipeline's ``encode_meshes``}."""
    from bench_common import B_MAX, B_MIN, RESOLUTIONS, build_netc, build_netg
    from monoport_amd import pipeline
    from monoport_amd.recon import pifu_calib
    dev = torch.device(DEV)
    netg, netc = build_netg(dev)[0], build_netc(dev)
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(dev)
    planes_hwc = planes.permute(1, 2, 0).contiguous()

    def hook(feat):  # the bench's synthetic-data hook: channels 0 / 1 are the body's depth planes
        feat[:, 0:2].copy_(planes[None].expand(feat.shape[0], -1, -1, -1))

    def hook_hwc(feat_hwc):
        feat_hwc[..., 0:2].copy_(planes_hwc[None].expand(feat_hwc.shape[0], -1, -1, -1))

    hook.hwc = hook_hwc
    images = torch.stack([torch.from_numpy(syn.synthetic_image(f % 8)) for f in range(frames)]).to(dev)
    calibs = torch.cat([pifu_calib(*syn.scene_camera(3 * f), device=DEV) for f in range(frames)])
    pipes, cameras = {}, {}
    for name, mesh, *pictures in meshes:
        kw = dict(pictures=pictures[0]) if pictures else {}
        if len(pictures) > 2:  # further keywords of the slot (lighting=)
            kw.update(pictures[2])
        kw.pop("encode_pictures", None)
        cameras[name] = dict(cameras=pictures[1]) if pictures else {}
        pipes[name] = pipeline.FramePipeline(netg, dev, depth=depth, batch=frames, resolutions=RESOLUTIONS,
                                             b_min=B_MIN, b_max=B_MAX, feature_hook=hook, use_graph=True,
                                             netC=netc, mesh=mesh, **kw)
        if len(pictures) > 2 and "encode_pictures" in pictures[2]:  # --jpeg: files behind the pictures
            pipes[name].encode_pictures(pictures[2]["encode_pictures"])
        if glbs and name in glbs:
            pipes[name].encode_meshes(glbs[name])
        pipes[name].prepare()

    def fn(name, consume=None):
        def run():
            for s in [pipes[name].submit(images, calibs, **cameras[name]) for _ in range(depth)]:
                got = consume(s) if consume else (s.pictures() if cameras[name] else s.meshes())
                assert all(m is not None for m in got)
        return run
    return pipes, fn


def slot_mesh_batch(a, frames=20):
    """A slot of ``frames`` frames with mesh output, pipeline.MESH_BATCH at 1 / 4 / all, per-frame ms of a submission
    (wait and the one host read of ``meshes()`` included); alone and as three slots submitted back to back."""
    from bench_common import B_MAX, B_MIN, RESOLUTIONS, build_netc, build_netg
    from monoport_amd import pipeline
    from monoport_amd.recon import pifu_calib
    dev = torch.device(DEV)
    netg, netc = build_netg(dev)[0], build_netc(dev)
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(dev)
    planes_hwc = planes.permute(1, 2, 0).contiguous()

    def hook(feat):  # the bench's synthetic-data hook: channels 0 / 1 are the body's depth planes
        feat[:, 0:2].copy_(planes[None].expand(feat.shape[0], -1, -1, -1))

    def hook_hwc(feat_hwc):
        feat_hwc[..., 0:2].copy_(planes_hwc[None].expand(feat_hwc.shape[0], -1, -1, -1))

    hook.hwc = hook_hwc
    images = torch.stack([torch.from_numpy(syn.synthetic_image(f % 8)) for f in range(frames)]).to(dev)
    calibs = torch.cat([pifu_calib(*syn.scene_camera(3 * f), device=DEV) for f in range(frames)])
    out = {"frames_per_slot": frames, "unit": "ms per frame", "normals": "accumulate", "colors": True}
    pictures = dict(views=4, res=257, shade="normals", projection="perspective", nearest="min", near=2.5,
                    perspective_correct=True)
    cameras = torch.eye(4).repeat(4, 1, 1)
    cameras[:, 0, 0] = cameras[:, 1, 1] = 2.5
    cameras[:, 0, 3] = torch.tensor([-0.3, -0.1, 0.1, 0.3])
    cameras[:, 2, 3] = 3.0  # the box at z = 2 .. 4: the plane at 2.5 cuts the body
    out["pictures"] = pictures
    for depth in (1, 3):
        pipes = {}
        for name, mesh in (("mesh", {"normals": "accumulate"}), ("no_mesh", None), ("pictures", {"normals": "accumulate"})):
            pipes[name] = pipeline.FramePipeline(netg, dev, depth=depth, batch=frames, resolutions=RESOLUTIONS,
                                                 b_min=B_MIN, b_max=B_MAX, feature_hook=hook, use_graph=True,
                                                 netC=netc, mesh=mesh, pictures=pictures if name == "pictures" else None)
            pipes[name].prepare()

        def run(name, mesh_batch):
            def fn():
                pipeline.MESH_BATCH = mesh_batch
                kw = dict(cameras=cameras) if name == "pictures" else {}
                slots = [pipes[name].submit(images, calibs, **kw) for _ in range(depth)]
                for s in slots:
                    if name == "pictures":
                        assert all(p_ is not None for p_ in s.pictures())
                    elif name == "mesh":
                        assert all(m is not None for m in s.meshes())
                    else:
                        s.wait()
            return fn

        ways = {"mesh_batch_1": run("mesh", 1), "mesh_batch_4": run("mesh", 4), "mesh_batch_all": run("mesh", frames),
                "no_mesh": run("no_mesh", 4), "mesh_pictures_batch_all": run("pictures", frames)}
        res = alternate(ways, a.passes, frames * depth)
        res["pictures_add_ms"] = round(res["mesh_pictures_batch_all"]["median_ms"] - res["mesh_batch_all"]["median_ms"], 4)
        pic = pipes["pictures"].slots[0].pictures()[0]
        res["picture_covered_pixels"] = [int((pic.face[v] >= 0).sum().item()) for v in range(4)]
        m = pipes["mesh"].slots[0].meshes()[0]
        res["vertices"], res["faces"] = int(m.verts.shape[0]), int(m.faces.shape[0])
        out["depth%d" % depth] = res
        for p_ in pipes.values():
            p_.close()
        del pipes
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
