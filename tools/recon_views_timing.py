"""A multi-view (V = 3) 17..257 reconstruction of the body fixture through Seg3dLossless, two engines in ONE process
on one MI355X: (a) the default engine, which serves a multi-view query_func level by level (ops.recon_generic),
and (b) fuse_views=True (ops.recon_views, one asynchronous C-ABI call).  Both validate="always" unless asked otherwise.

    python tools/recon_views_timing.py [--passes 5] [--recons 20] [--views 3] [--validate always|first]

(``--validate first``: after its first calls the fused engine trusts the binding and skips the validation query of
the coarsest level, except on every REVALIDATE_EVERY-th call; the default engine is not affected.)

After a warm-up of both, the passes of (a) and (b) alternate; a pass is `recons` reconstructions, wall clock around a
final stream sync.  Prints one JSON line: per engine the median, minimum and maximum time per reconstruction (ms)
over the passes, and -- from a separate pair of passes bracketed by mp_profile_begin / mp_profile_end, outside the
timed ones -- the summed GPU time of the multi-view kernel launches of one reconstruction.  The verdict fields
restate the acceptance rule: (b)'s median below (a)'s by more than the larger min-max spread, and (b)'s summed
kernel time not above (a)'s by more than that spread.

    python tools/recon_views_timing.py --frames N [--passes 5] [--reps 1] [--views 3] [--out FILE]

N frames of V views (the body maps in an order rotated per frame, the cameras 7 degrees further round the orbit per
frame) reconstructed (a) by N sequential ops.recon_views calls on one stream and (b) by ops.recon_views_batch, one
call per chunk of ops.max_view_frames(V) frames.  After a warm-up of both the passes alternate; a pass is all N
frames `reps` times over (a small N alone is too short a window), wall clock around a stream sync.  One JSON line
(appended to FILE with --out): per side the median, minimum and maximum ms per repetition of the N frames, the per-level GPU time of the multi-view kernel launches (mp_profile_*, a separate pass each:
(a)'s N launches of a level summed), whether every frame's volume and status are equal, and the verdicts: (b)'s
median no worse than (a)'s plus (a)'s own min-max spread, and (b)'s last-level kernel time per frame within that
spread of (a)'s (and, separately, not above it: one launch over all frames has one tail where N launches have N).
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
from monoport_amd.implicit_seg.functional import Seg3dLossless  # noqa: E402
from monoport_amd.modeling import PIFuNetG, heads  # noqa: E402
from oracle import pifu_oracle as orc  # noqa: E402

DEV = "cuda:0"
RES = [17, 33, 65, 129, 257]


def build_net(v_n):
    net = PIFuNetG()
    net.surface_classifier = heads.SurfaceClassifier(heads.PIFuNetGMLP().filter_channels, v_n, False, "sigmoid")
    with torch.no_grad():
        for i, (w, b) in enumerate(syn.body_mlp("G", noise=0.05, seed=251)):
            net.surface_classifier.filters[i].weight.copy_(torch.from_numpy(w)[:, :, None])
            net.surface_classifier.filters[i].bias.copy_(torch.from_numpy(b))
    return net.to(DEV).eval()


def frames_mode(a):
    """--frames N: sequential ops.recon_views against ops.recon_views_batch (module docstring)."""
    v_n, n = a.views, a.frames
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=251), syn.LAST_OP["G"])
    m = [ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 252 + v))[None].to(DEV)) for v in range(v_n)]
    maps = [[m[(v + f) % v_n] for v in range(v_n)] for f in range(n)]
    calibs = torch.from_numpy(np.stack([[orc.pifu_calib(*syn.scene_camera(6 * v + 7 * f))[0] for v in range(v_n)]
                                        for f in range(n)])).to(DEV)
    lo, hi = [-1.0] * 3, [1.0] * 3
    step = ops.max_view_frames(v_n)
    volumes = [torch.empty((RES[-1],) * 3, dtype=torch.float32, device=DEV) for _ in range(n)]
    status = torch.zeros((n, 1 + len(RES)), dtype=torch.int32, device=DEV)

    def sequential():
        return [ops.recon_views(mlp, maps[f], calibs[f], "orthogonal", syn.Z_SCALE, lo, hi, RES) for f in range(n)]

    def batched():
        for f0 in range(0, n, step):
            f1 = min(f0 + step, n)
            ops.recon_views_batch(mlp, maps[f0:f1], calibs[f0:f1], "orthogonal", syn.Z_SCALE, lo, hi, RES,
                                  volumes=volumes[f0:f1], status=status[f0:f1])

    sides = {"sequential": sequential, "batched": batched}
    ref = sequential()
    batched()
    torch.cuda.synchronize()
    same = all(torch.equal(v, r[0]) for v, r in zip(volumes, ref)) and status.tolist() == [r[1].tolist() for r in ref]
    counts = status.tolist()
    del ref
    for fn in sides.values():  # warm-up of both
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in sides}
    for _ in range(a.passes):
        for name, fn in sides.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.reps)
    levels = {}
    for name, fn in sides.items():  # event-bracketed launches, outside the timed passes
        torch.cuda.synchronize()
        ops.profile_begin(DEV)
        fn()
        torch.cuda.synchronize()
        ms = ops.profile_end(DEV)
        assert ms.size % len(RES) == 0, "expected one launch per level and call, got %d" % ms.size
        levels[name] = [round(float(t), 4) for t in ms.reshape(-1, len(RES)).sum(0)]
    out = {"mode": "frames", "V": v_n, "frames": n, "frames_per_call": step, "resolutions": RES, "passes": a.passes,
           "reps_per_pass": a.reps, "equal": bool(same), "status_first": counts[0], "status_last": counts[-1]}
    for name in sides:
        t = np.array(times[name])
        out[name] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                     "max_ms": round(float(t.max()), 4), "per_pass_ms": [round(float(x), 4) for x in t],
                     "level_kernel_ms": levels[name], "kernel_sum_ms": round(sum(levels[name]), 4)}
    spread = out["sequential"]["max_ms"] - out["sequential"]["min_ms"]
    out["sequential_spread_ms"] = round(spread, 4)
    out["batched_no_worse_than_sequential_plus_spread"] = bool(
        out["batched"]["median_ms"] <= out["sequential"]["median_ms"] + spread)
    last = [levels[name][-1] / n for name in ("sequential", "batched")]
    out["last_level_kernel_ms_per_frame"] = {"sequential": round(last[0], 4), "batched": round(last[1], 4)}
    # spread / n: the spread of a pass is that of n frames
    out["last_level_per_frame_within_spread"] = bool(abs(last[1] - last[0]) <= spread / n)
    out["last_level_per_frame_not_above_sequential_plus_spread"] = bool(last[1] <= last[0] + spread / n)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--recons", type=int, default=20)
    ap.add_argument("--views", type=int, default=3)
    ap.add_argument("--validate", default="always", choices=["always", "first"])
    ap.add_argument("--frames", type=int, default=0, help="N > 0: sequential recon_views against recon_views_batch")
    ap.add_argument("--reps", type=int, default=1, help="--frames: repetitions of the N frames per pass")
    ap.add_argument("--out", default=None, help="--frames: append the JSON line to this file")
    a = ap.parse_args()
    if a.frames > 0:
        return frames_mode(a)
    v_n = a.views
    net = build_net(v_n)
    f = np.stack([syn.body_feat(256, 128, 128, 252 + v) for v in range(v_n)])
    feats = [[torch.from_numpy(f).to(DEV)]]
    calib = torch.from_numpy(np.stack([orc.pifu_calib(*syn.scene_camera(6 * v))[0] for v in range(v_n)])).to(DEV)

    def query_func(points, im_feat_list, calib_tensor):
        samples = points.repeat(v_n, 1, 1).permute(0, 2, 1)
        return net.query(im_feat_list, points=samples, calibs=calib_tensor)[0][:1]

    def make(**kw):
        return Seg3dLossless(query_func=query_func, b_min=np.array([[-1.0, -1, -1]]), b_max=np.array([[1.0, 1, 1]]),
                             resolutions=RES, balance_value=0.5, faster=True, validate=a.validate, **kw).to(DEV)
    engines = {"generic": make(), "fused": make(fuse_views=True)}

    def run(name, n):
        eng = engines[name]
        for _ in range(n):
            vol = eng(im_feat_list=feats, calib_tensor=calib)
        assert vol is not None and eng.last_path == name
        return vol

    vols = {name: run(name, 3).clone() for name in engines}  # warm-up of both
    torch.cuda.synchronize()
    same = bool(torch.equal(vols["generic"], vols["fused"]))
    times = {name: [] for name in engines}
    for _ in range(a.passes):
        for name in engines:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, a.recons)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.recons)
    kern = {}
    for name in engines:  # event-bracketed launches, outside the timed passes
        torch.cuda.synchronize()
        ops.profile_begin(DEV)
        run(name, 1)
        torch.cuda.synchronize()
        ms = ops.profile_end(DEV)
        kern[name] = {"launches": int(ms.size), "sum_ms": round(float(ms.sum()), 4),
                      "per_launch_ms": [round(float(t), 4) for t in ms]}
    out = {"V": v_n, "validate": a.validate, "resolutions": RES, "passes": a.passes, "recons_per_pass": a.recons,
           "volumes_equal": same, "status": engines["fused"].last_status.tolist()}
    spread = 0.0
    for name in engines:
        t = np.array(times[name])
        out[name] = {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4),
                     "max_ms": round(float(t.max()), 4), "kernels": kern[name]}
        spread = max(spread, float(t.max() - t.min()))
    out["larger_spread_ms"] = round(spread, 4)
    out["fused_faster_by_more_than_spread"] = bool(
        out["generic"]["median_ms"] - out["fused"]["median_ms"] > spread)
    out["fused_kernel_time_within_spread"] = bool(
        kern["fused"]["sum_ms"] <= kern["generic"]["sum_ms"] + spread)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
