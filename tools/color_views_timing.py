"""What multi-view netC colours cost on one MI355X: the V = 3 body fixture at 17..257, netC colours on the mesh.

    python tools/color_views_timing.py [--views 3] [--frames 4 21] [--slot-batch 4] [--passes 5] [--reps 3] [--out FILE]

(a) The colour query alone.  N frames are reconstructed (ops.recon_views_batch), meshed (ops.marching_cubes_raw_batch)
and turned into query points (ops.mesh_points_raw_batch) once, outside the timing.  Then, on one stream:
  * sequential: N ops.query_views calls on the first count_f points of each frame, counts known on the host -- what a
    user of a multi-view netC does today (mesh_util.vertex_colors per mesh);
  * batched: ops.query_views_counted_batch, one call per chunk of ops.max_view_frames(V) frames, counts on the device.
(b) The slot.  A pipeline.ColorViewsSlot step (submit + meshes(), mesh={"colors": True}) against the same step of a
pipeline.ViewsSlot with uncoloured meshes, same images and cameras: the difference is what colours cost per frame
(netC's encoder pass, the textured render and the mesh colours).

Method for both: a warm-up of both sides, then `passes` alternating passes, wall clock around a stream sync; a pass is
`reps` repetitions.  One JSON line per measurement (appended to FILE with --out): per side the median, minimum and
maximum ms, the per-pass values, and for (a) whether the batched bits equal the sequential ones.
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
from monoport_amd import ops, synthetic as syn  # noqa: E402
from monoport_amd.modeling import PIFuNetC, PIFuNetG, heads  # noqa: E402
from oracle import pifu_oracle as orc  # noqa: E402

DEV = "cuda:0"
RES = [17, 33, 65, 129, 257]
LO, HI = [-1.0] * 3, [1.0] * 3


def alternate(sides, passes, reps):
    for fn in sides.values():  # warm-up of both
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in sides}
    for _ in range(passes):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / reps)
    out = {}
    for name, t in times.items():
        t = np.array(t)
        out[name] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                     "max_ms": round(float(t.max()), 4), "per_pass_ms": [round(float(x), 4) for x in t]}
    return out


def emit(out, path):
    line = json.dumps(out)
    print(line, flush=True)
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def camera_sets(n, v_n):
    return torch.from_numpy(np.stack([[orc.pifu_calib(*syn.scene_camera(6 * v + 7 * f))[0] for v in range(v_n)]
                                      for f in range(n)])).to(DEV)


def query_mode(a, n):
    """(a): N sequential ops.query_views calls against ops.query_views_counted_batch."""
    v_n, view = a.views, 0
    mlp_g = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=251), syn.LAST_OP["G"])
    mlp_c = ops.PackedMLP.from_layers(DEV, syn.rand_mlp("C", 61, 2.0), syn.LAST_OP["C"])
    g = [ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 252 + v))[None].to(DEV)) for v in range(v_n)]
    c = [ops.pack_features(torch.from_numpy(syn.rand_feat(512, 128, 128, 262 + v))[None].to(DEV)) for v in range(v_n)]
    maps_g = [[g[(v + f) % v_n] for v in range(v_n)] for f in range(n)]
    maps_c = [[c[(v + f) % v_n] for v in range(v_n)] for f in range(n)]
    calibs = camera_sets(n, v_n)
    step = ops.max_view_frames(v_n)
    points, counts = [], []
    for f0 in range(0, n, 4):  # four 257^3 volumes at a time: only the points stay
        f1 = min(f0 + 4, n)
        vols, status = ops.recon_views_batch(mlp_g, maps_g[f0:f1], calibs[f0:f1], "orthogonal", syn.Z_SCALE, LO, HI, RES)
        raws = ops.marching_cubes_raw_batch(vols, 0.5, LO, HI)
        for p, k in ops.mesh_points_raw_batch([r[0] for r in raws], [r[2] for r in raws]):
            points.append(p.clone())
            counts.append(k.clone())
        assert all(int(s[0]) == 1 for s in status.tolist())
    host = [int(k.item()) for k in counts]
    cap = points[0].shape[1]
    assert max(host) <= cap
    views = [p[:, :k][None].expand(v_n, 3, k) for p, k in zip(points, host)]
    outs = [torch.zeros((3, cap), dtype=torch.float32, device=DEV) for _ in range(n)]

    def sequential():
        return [ops.query_views(mlp_c, maps_c[f], views[f], calibs[f], "orthogonal", syn.Z_SCALE)[view] for f in range(n)]

    def batched():
        for f0 in range(0, n, step):
            f1 = min(f0 + step, n)
            ops.query_views_counted_batch(mlp_c, maps_c[f0:f1], points[f0:f1], counts[f0:f1], calibs[f0:f1], "orthogonal",
                                          syn.Z_SCALE, view=view, outs=outs[f0:f1])

    ref = sequential()
    batched()
    torch.cuda.synchronize()
    same = all(torch.equal(o[:, :k].view(torch.int32), r.view(torch.int32)) for o, r, k in zip(outs, ref, host))
    del ref
    out = {"mode": "query", "V": v_n, "frames": n, "frames_per_call": step, "view": view, "capacity": cap,
           "points_min": min(host), "points_max": max(host), "points_sum": sum(host), "equal": bool(same),
           "passes": a.passes, "reps_per_pass": a.reps}
    out.update(alternate({"sequential": sequential, "batched": batched}, a.passes, a.reps))
    spread = out["sequential"]["max_ms"] - out["sequential"]["min_ms"]
    out["sequential_spread_ms"] = round(spread, 4)
    out["batched_faster_by_more_than_spread"] = bool(out["sequential"]["median_ms"] - out["batched"]["median_ms"] > spread)
    emit(out, a.out)


def build_net(kind, v_n, seed):
    net = PIFuNetG() if kind == "G" else PIFuNetC()
    ch = heads.PIFuNetGMLP().filter_channels if kind == "G" else heads.PIFuNetCMLP().filter_channels
    net.surface_classifier = heads.SurfaceClassifier(ch, v_n, False, "sigmoid" if kind == "G" else "tanh")
    layers = syn.body_mlp("G", noise=0.05, seed=251) if kind == "G" else syn.rand_mlp("C", 61, 2.0)
    with torch.no_grad():
        for i, (w, b) in enumerate(layers):
            net.surface_classifier.filters[i].weight.copy_(torch.from_numpy(w)[:, :, None])
            net.surface_classifier.filters[i].bias.copy_(torch.from_numpy(b))
    shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
    net.image_filter.load_state_dict({k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(shapes, seed).items()})
    return net.to(DEV).eval()


def body_hook():
    """Channels 0 / 1 of every netG map are the body's depth planes (the benchmark's synthetic-data hook)."""
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(DEV)
    planes_hwc = planes.permute(1, 2, 0).contiguous()

    def hook(feat):
        feat[:, 0:2].copy_(planes[None].expand(feat.shape[0], -1, -1, -1))

    def hook_hwc(feat_hwc):
        feat_hwc[..., 0:2].copy_(planes_hwc[None].expand(feat_hwc.shape[0], -1, -1, -1))

    hook.hwc = hook_hwc
    return hook


def slot_mode(a):
    """(b): a ColorViewsSlot step with coloured meshes against a ViewsSlot step with uncoloured ones."""
    from monoport_amd.pipeline import ColorViewsSlot, ViewsSlot
    v_n, n = a.views, a.slot_batch
    net_g, net_c = build_net("G", v_n, 71), build_net("C", v_n, 72)
    images = torch.from_numpy(np.stack([[syn.synthetic_image(10 * f + v) for v in range(v_n)] for f in range(n)])).to(DEV)
    calibs = camera_sets(n, v_n)
    kw = dict(batch=n, resolutions=RES, b_min=LO, b_max=HI, feature_hook=body_hook())
    plain = ViewsSlot(net_g, torch.device(DEV), mesh={"normals": "accumulate"}, **kw)
    colour = ColorViewsSlot(net_g, torch.device(DEV), netC=net_c, mesh={"normals": "accumulate", "colors": True}, **kw)
    found = {}

    def step(slot, name):
        def run():
            slot.submit(images, calibs)
            found[name] = slot.meshes()
        return run

    try:
        out = {"mode": "slot", "V": v_n, "frames": n, "passes": a.passes, "reps_per_pass": a.reps}
        out.update(alternate({"views_slot": step(plain, "plain"), "color_views_slot": step(colour, "colour")},
                             a.passes, a.reps))
        assert all(m is not None and m.colors is not None for m in found["colour"])
        assert all(torch.equal(p.verts, c.verts) for p, c in zip(found["plain"], found["colour"]))
        out["vertices"] = [int(m.verts.shape[0]) for m in found["colour"]]
        out["status"] = colour.status.tolist()
        d = out["color_views_slot"]["median_ms"] - out["views_slot"]["median_ms"]
        out["colours_ms_per_step"] = round(d, 4)
        out["colours_ms_per_frame"] = round(d / n, 4)
        emit(out, a.out)
    finally:
        plain.close()
        colour.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--frames", type=int, nargs="*", default=[4, 21], help="(a): the frame counts N; none: skip (a)")
    ap.add_argument("--slot-batch", type=int, default=4, help="(b): frames of the slot; 0: skip (b)")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    a = ap.parse_args()
    for n in a.frames:
        query_mode(a, n)
    if a.slot_batch > 0:
        slot_mode(a)


if __name__ == "__main__":
    main()
