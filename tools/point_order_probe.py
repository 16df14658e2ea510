"""Does the order of an octree level's point list matter to the table query kernel?

One benchmark frame set (20 frames: the F-body head, cameras scene_camera(3 s), 128^2 maps with registered skip
tables, 17-33-65-129-257 lattice) is reconstructed level by level through ``LevelEngine`` (mp_octree_select_box /
mp_lattice_points), which yields every level's node list in the order select_compact_kernel writes it.  For the
levels given with ``--levels`` the 20 lists go through ONE table query launch (``ops.query_counted_batch``), timed
with HIP events on one stream: once in selection order, once permuted on the host by the texel cell
(y0 * W + x0 of the first bilinear tap) each point samples.  Both orders alternate, 5 repetitions after warm-up;
the un-permuted outputs must be ``array_equal``.

Decision rule printed per level: the sorted order wins only if its median beats the unsorted median by more than
twice the largest difference between two unsorted repetitions.

    python tools/point_order_probe.py [--out profiles/point_order_probe.txt] [--levels 2 3 4] [--frames 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from monoport_amd import ops, synthetic as syn  # noqa: E402
from monoport_amd.recon import pifu_calib  # noqa: E402

RES = [17, 33, 65, 129, 257]
B_MIN, B_MAX = [-1.0] * 3, [1.0] * 3
H = W = 128
REPS, WARM = 5, 2


def texel_keys(pts, calib):
    """[n,3] world points, [4,4] calibration -> y0 * W + x0 of tap 0 (float32 restatement of make_taps; points
    outside the image go to the last bin H * W)."""
    c = calib.astype(np.float32)
    x = (pts @ c[0, :3] + c[0, 3]).astype(np.float32)
    y = (pts @ c[1, :3] + c[1, 3]).astype(np.float32)
    ix = (x + np.float32(1)) * np.float32(0.5) * np.float32(W - 1)
    iy = (y + np.float32(1)) * np.float32(0.5) * np.float32(H - 1)
    x0 = np.clip(np.floor(ix), 0, W - 1).astype(np.int64)
    y0 = np.clip(np.floor(iy), 0, H - 1).astype(np.int64)
    inside = (x >= -1) & (x <= 1) & (y >= -1) & (y <= 1)
    return np.where(inside, y0 * W + x0, H * W)


def cells_per_tile(keys, tile=32):
    """Mean number of distinct texel cells per ``tile`` consecutive entries."""
    n = keys.shape[0] // tile * tile
    if n == 0:
        return float("nan")
    k = np.sort(keys[:n].reshape(-1, tile), axis=1)
    return float((1 + (np.diff(k, axis=1) != 0).sum(1)).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles",
                                                  "point_order_probe.txt"))
    ap.add_argument("--levels", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--frames", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda:0"
    nf = args.frames
    mlp = ops.PackedMLP.from_layers(dev, syn.body_mlp("G", noise=0.05, seed=1), syn.LAST_OP["G"])
    feats = torch.stack([ops.pack_features(torch.from_numpy(syn.body_feat(256, H, W, s % 8))[None].to(dev))
                         for s in range(nf)]).contiguous()
    maps = [feats[s] for s in range(nf)]
    calibs = [pifu_calib(*syn.scene_camera(3 * s), device=dev) for s in range(nf)]
    handle = ops.skip_table_batch(mlp, feats)

    # every frame's lists, level by level (the engine's own selection kernels; values through the table kernel)
    lists = {l: [] for l in args.levels}
    for s in range(nf):
        eng = ops.LevelEngine(dev, B_MIN, B_MAX, RES)
        for l in range(len(RES)):
            pts = eng.select()
            if pts is None:
                raise SystemExit("frame %d: level %d selected nothing" % (s, l))
            if l in lists:
                lists[l].append(pts.clone())
            eng.scatter(ops.query(mlp, maps[s], pts.t()[None], calibs[s], syn.Z_SCALE))

    lines = ["point_order_probe: %d frames, one table query launch per level, %d repetitions after %d warm-up, "
             "orders alternating; ms per launch" % (nf, REPS, WARM),
             "level  res  points    cells/tile sel -> texel   unsorted ms (min..max, spread)      sorted ms (min..max)"
             "       gain ms (rule: > 2 x spread)"]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for l in args.levels:
        n = [int(p.shape[0]) for p in lists[l]]
        cap = max(n)
        counts = [torch.tensor([k], dtype=torch.int32, device=dev) for k in n]
        sel, tex, perms, c_sel, c_tex = [], [], [], [], []
        for s in range(nf):
            p = lists[l][s].cpu().numpy()
            keys = texel_keys(p, calibs[s][0].cpu().numpy())
            perm = np.argsort(keys, kind="stable")
            perms.append(perm)
            c_sel.append(cells_per_tile(keys))
            c_tex.append(cells_per_tile(keys[perm]))
            for dst, q in ((sel, p), (tex, p[perm])):
                buf = torch.zeros((3, cap), dtype=torch.float32, device=dev)
                buf[:, :n[s]] = torch.from_numpy(np.ascontiguousarray(q.T)).to(dev)
                dst.append(buf)
        outs = {k: [torch.zeros((mlp.cout, cap), dtype=torch.float32, device=dev) for _ in range(nf)]
                for k in ("sel", "tex")}
        ms = {"sel": [], "tex": []}
        for rep in range(WARM + REPS):
            for k, pts in (("sel", sel), ("tex", tex)):
                ev[0].record()
                ops.query_counted_batch(mlp, maps, pts, counts, calibs, syn.Z_SCALE, outs=outs[k])
                ev[1].record()
                ev[1].synchronize()
                if rep >= WARM:
                    ms[k].append(ev[0].elapsed_time(ev[1]))
        for s in range(nf):
            a = outs["sel"][s][:, :n[s]].cpu().numpy()
            b = np.empty_like(a)
            b[:, perms[s]] = outs["tex"][s][:, :n[s]].cpu().numpy()
            if not np.array_equal(a, b):
                raise SystemExit("level %d frame %d: the permuted launch computed other values" % (l, s))
        u, t = np.array(ms["sel"]), np.array(ms["tex"])
        spread = float(u.max() - u.min())
        gain = float(np.median(u) - np.median(t))
        lines.append("%5d  %3d  %7d   %6.1f -> %5.1f            %.4f (%.4f..%.4f, %.4f)      %.4f (%.4f..%.4f)"
                     "     %+.4f  %s" % (l, RES[l], sum(n), np.mean(c_sel), np.mean(c_tex), np.median(u), u.min(),
                                         u.max(), spread, np.median(t), t.min(), t.max(), gain,
                                         "SORT" if gain > 2 * spread else "no"))
        lines.append("       unsorted %s   sorted %s" % (" ".join("%.4f" % v for v in u), " ".join("%.4f" % v for v in t)))
    handle.release()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
