"""The coloured mesh of the 257^3 body volume, three ways in ONE process on one MI355X:

  (a) recon.marching_cubes + mesh_util.vertex_colors  (two host round trips: the counts, then the colour query)
  (b) recon.reconstruct_mesh(normals=None, netC=...)   (one device chain, one host sync)
  (c) recon.reconstruct_mesh(normals="accumulate", netC=...)   ((b) plus the per-vertex normals)
  (d) as (c) with normals="reference"

    python tools/mesh_timing.py [--passes 5] [--meshes 20] [--out profiles/mesh_timing.json]

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
from monoport_amd.recon import marching_cubes, reconstruct_mesh  # noqa: E402
from oracle import pifu_oracle as orc  # noqa: E402

DEV = "cuda:0"
RES = [17, 33, 65, 129, 257]
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--meshes", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_timing.json"))
    a = ap.parse_args()
    mlp = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), 1)
    fh = ops.pack_features(torch.from_numpy(syn.body_feat(256, 128, 128, 2))[None].to(DEV))
    cal = torch.from_numpy(orc.pifu_calib(*syn.scene_camera(30))).to(DEV)
    vol, status = ops.recon(mlp, fh, cal, syn.Z_SCALE, BMIN, BMAX, RES)
    assert int(status[0].item()) == 1
    vol = vol[None, None]
    netC = PIFuNetC()
    with torch.no_grad():
        for i, (w, b) in enumerate(syn.rand_mlp("C", 61, 2.0)):
            netC.surface_classifier.filters[i].weight.copy_(torch.from_numpy(w)[:, :, None])
            netC.surface_classifier.filters[i].bias.copy_(torch.from_numpy(b))
    netC.surface_classifier.to(DEV)
    netC.eval()
    feat_C = [[torch.from_numpy(syn.rand_feat(512, 128, 128, 62))[None].to(DEV)]]
    calib = torch.eye(4, device=DEV)[None]

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
    line = json.dumps(out)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh_:
        fh_.write(line + "\n")


if __name__ == "__main__":
    main()
