"""The multi-view query (mp_query_views, csrc/query_views.hip) against mp_query_batch over the same V maps and
points on the plain kernels (no skip tables registered), V in {2,3,4,8}, 250 k points.  The two calls alternate in
one process after a warm-up; each time is the median of REPS launches bracketed by device events.  One JSON line
per V: times, their ratio (target <= 1.05), executed MFMA FLOP/s and its share of the f32 MFMA roof.

    python tools/query_views_probe.py [--reps 25] [--n 250000]

Kernel times for the same launches come from a separate run under ``rocprofv3 --kernel-trace --stats``.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monoport_amd import ops, synthetic as syn  # noqa: E402
from oracle import pifu_oracle as orc  # noqa: E402

F32_MFMA_ROOF = 157e12  # v_mfma_f32_32x32x2_f32 peak of the chip (query.hip header)
# MFMA MACs per column (point or (point, view) pair) of the netG head: layers 0-3 incl. the skip segments and z
MACS_COL = 1024 * 257 + 512 * (1024 + 257) + 256 * (512 + 257) + 128 * (256 + 257)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--n", type=int, default=250000)
    ap.add_argument("--views", default="2,3,4,8")
    a = ap.parse_args()
    dev = "cuda:0"
    mlp = ops.PackedMLP.from_layers(dev, syn.body_mlp("G", noise=0.05, seed=1), syn.LAST_OP["G"])
    for v_n in [int(v) for v in a.views.split(",")]:
        fh = [ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 10 + v))[None].to(dev))
              for v in range(v_n)]
        cal = torch.from_numpy(np.stack([orc.pifu_calib(*syn.scene_camera(40 * v))[0] for v in range(v_n)])).to(dev)
        pts = torch.from_numpy(syn.rand_points(a.n, 7, 1.0))[None].to(dev).repeat(v_n, 1, 1)
        out_v = torch.empty((v_n, 1, a.n), device=dev)
        out_b = torch.empty((v_n, 1, a.n), device=dev)

        def views():
            ops.query_views(mlp, fh, pts, cal, "orthogonal", syn.Z_SCALE, out=out_v)

        def batch():
            ops.query_batch(mlp, fh, pts, cal, ["orthogonal"] * v_n, syn.Z_SCALE, out=out_b)

        for _ in range(3):
            views()
            batch()
        torch.cuda.synchronize()
        ts = {"views": [], "batch": []}
        for _ in range(a.reps):
            for name, fn in (("views", views), ("batch", batch)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts[name].append(e0.elapsed_time(e1))
        t_v, t_b = float(np.median(ts["views"])), float(np.median(ts["batch"]))
        cols_v = -(-a.n // (64 // v_n)) * 64  # executed columns: G = 64 // V points per 64-column tile
        cols_b = v_n * -(-a.n // 64) * 64
        fl_v, fl_b = 2.0 * MACS_COL * cols_v / (t_v * 1e-3), 2.0 * MACS_COL * cols_b / (t_b * 1e-3)
        print(json.dumps({"V": v_n, "n": a.n, "views_ms": round(t_v, 4), "batch_ms": round(t_b, 4),
                          "ratio": round(t_v / t_b, 4), "views_tflops": round(fl_v / 1e12, 2),
                          "views_roof": round(fl_v / F32_MFMA_ROOF, 3), "batch_tflops": round(fl_b / 1e12, 2),
                          "batch_roof": round(fl_b / F32_MFMA_ROOF, 3), "dead_columns": round(1 - v_n * (64 // v_n) / 64, 3)}),
              flush=True)


if __name__ == "__main__":
    main()
