"""What the fixed-budget engine (mp_recon_topk_batch, csrc/topk.hip) costs and gives on the 257^3 body scene, next to
the lossless call, in ONE process on one MI355X:

  - per level 33 .. 257: the selection of mp_octree_select_topk (upsample + three histogram / scan passes + tie
    count / scan + emit) at the 1/2 budget, the upsample alone (mp_octree_select_box, box 0) and the lossless
    selection (upsample + dilate + compact), HIP events around `--calls` calls; previous level = the lossless
    volume of that level, every node of it evaluated;
  - the whole reconstruction per frame, one frame per call and 20 frames per call: ops.recon(_batch) and
    ops.recon_topk(_batch) with budgets of 1/4, 1/2 and 1x the lossless per-level counts; the passes alternate, a
    pass is `--frames` frames, wall clock around a final stream sync;
  - IoU of each thresholded volume against the lossless one, and the points per level.

    python tools/topk_timing.py [--passes 5] [--frames 20] [--calls 50] [--out profiles/topk_timing.json]

Prints (and writes) one JSON line.  The yardstick is the lossless call of the same run: the ratios are reported, not
asserted."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monoport_amd import ops, synthetic as syn  # noqa: E402
from oracle import pifu_oracle as orc  # noqa: E402

DEV = "cuda:0"
RES = [17, 33, 65, 129, 257]
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
FRACTIONS = {"quarter": 0.25, "half": 0.5, "full": 1.0}


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def selection_times(mlp, fh, cal, counts, calls):
    """ms per call of the three selections of every level >= 1 (HIP events around `calls` calls)."""
    ctx = ops.get_context(torch.device(DEV))
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    out = {}
    for l in range(1, len(RES)):
        rp, r = RES[l - 1], RES[l]
        prev, _ = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES[:l])
        prev = prev.contiguous()
        words_p, words = rp * rp * ((rp + 63) // 64), r * r * ((r + 63) // 64)
        ev_prev = torch.full((words_p,), -1, dtype=torch.int64, device=DEV)  # every node of the level before
        if rp % 64:
            ev_prev.view(rp * rp, -1)[:, -1] = (1 << (rp % 64)) - 1
        cur = torch.empty((r, r, r), dtype=torch.float32, device=DEV)
        ev_cur = torch.empty((words,), dtype=torch.int64, device=DEV)
        bnd = torch.empty((words,), dtype=torch.int64, device=DEV)
        packed = torch.empty((r ** 3,), dtype=torch.int32, device=DEV)
        count = torch.zeros((1,), dtype=torch.int32, device=DEV)
        k = max(counts[l] // 2, 1)

        def topk():
            ctx.check(ctx.lib.mp_octree_select_topk(ctx.handle, _p(prev), rp, _p(cur), r, _p(ev_prev), _p(ev_cur), k,
                                                    float("inf"), 0.5, _p(packed), _p(count), stream), "topk")

        def box(b):
            return lambda: ctx.check(ctx.lib.mp_octree_select_box(
                ctx.handle, _p(prev), rp, _p(cur), r, _p(ev_prev), _p(ev_cur), _p(bnd), b, 0.5, _p(packed),
                _p(count), stream), "box")

        ways = {"topk_select": topk, "upsample_only": box(0), "lossless_select": box({1: 9, 2: 7}.get(l, 3))}
        ms = {}
        for name, fn in ways.items():
            for _ in range(3):
                fn()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[name] = a.elapsed_time(b) / calls
        ms["topk_minus_upsample"] = ms["topk_select"] - ms["upsample_only"]
        ms["k"] = k
        out[str(r)] = ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_timing.json"))
    a = ap.parse_args()
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    fh = ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2))[None].to(DEV))
    cal = torch.from_numpy(orc.pifu_calib(*syn.scene_camera(30))).to(DEV)
    n = a.frames
    lossless, status = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES)
    counts = status.cpu().tolist()[1:]
    inside = lossless > 0.5
    budgets = {name: [0] + [max(int(c * f), 1) for c in counts[1:]] for name, f in FRACTIONS.items()}

    ways = {"lossless": lambda: ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES),
            "lossless_batch": lambda: ops.recon_batch(mlp, [fh] * n, [cal] * n, syn.Z_SCALE, BMIN, BMAX, RES)}
    for name, b in budgets.items():
        ways["topk_" + name] = lambda b=b: ops.recon_topk(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES, b)
        ways["topk_%s_batch" % name] = lambda b=b: ops.recon_topk_batch(mlp, [fh] * n, [cal] * n, syn.Z_SCALE, BMIN,
                                                                        BMAX, RES, b)
    quality = {}
    for name, b in budgets.items():
        vol, st = ops.recon_topk(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES, b)
        got = vol > 0.5
        quality[name] = {"budgets": b, "points": st.cpu().tolist()[1:],
                         "iou": float((got & inside).sum()) / float((got | inside).sum())}

    def run(name):
        if name.endswith("_batch"):
            ways[name]()
        else:
            for _ in range(n):
                ways[name]()

    for name in ways:  # warm-up of all
        run(name)
    torch.cuda.synchronize()
    times = {name: [] for name in ways}
    for _ in range(a.passes):
        for name in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / n)
    per_frame = {name: {"median": float(np.median(t)), "min": min(t), "max": max(t)} for name, t in times.items()}
    out = {"scene": "body 257^3", "resolutions": RES, "frames_per_pass": n, "passes": a.passes,
           "lossless_points": counts, "ms_per_frame": per_frame, "quality": quality,
           "ratio_to_lossless": {name: per_frame[name]["median"] /
                                 per_frame["lossless_batch" if name.endswith("_batch") else "lossless"]["median"]
                                 for name in ways if name.startswith("topk")},
           "selection_ms_per_level": selection_times(mlp, fh, cal, counts, a.calls)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
