"""Generate tests/golden/*.npz by running the REFERENCE's own Python modules.

Run in the build container only (needs /root/reference):

    python oracle/gen_golden.py

It imports monoport.lib.modeling.* and RTL/recon.py from /root/reference (never copied),
feeds them the seeded inputs of monoport_amd/synthetic.py and stores ONLY the reference outputs
(+ the seeds that regenerate the inputs).  The GPU box has no /root/reference: tests read the
committed fixtures.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("MONOPORT_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "refshim"), REF, os.path.join(REF, "RTL"), ROOT]

import torch  # noqa: E402

from monoport_amd import synthetic as syn  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def ref_net(kind):
    from monoport.lib.modeling.MonoPortNet import PIFuNetC, PIFuNetG
    torch.manual_seed(0)
    return (PIFuNetG() if kind == "G" else PIFuNetC()).eval()


def load_mlp(net, layers):
    sd = {}
    for i, (w, b) in enumerate(layers):
        sd["filters.%d.weight" % i] = torch.from_numpy(w)[:, :, None]
        sd["filters.%d.bias" % i] = torch.from_numpy(b)
    net.surface_classifier.load_state_dict(sd)


@torch.no_grad()
def gen_query():
    import recon as ref_recon
    from monoport.lib.modeling.geometry import orthogonal
    cases = {
        # name: (kind, mlp, feat, points, camera step)
        "query_G_rand": ("G", ("rand", 11, 2.0), ("rand", 256, 21), (49152, 31, 0.8), 33),
        "query_C_rand": ("C", ("rand", 12, 2.0), ("rand", 512, 22), (40960, 32, 0.8), 75),
        "query_G_body": ("G", ("body", 13, 0.05), ("body", 256, 23), (40960, 33, 0.7), 12),
    }
    for name, (kind, mlp, feat, pts, step) in cases.items():
        net = ref_net(kind)
        layers = (syn.rand_mlp(kind, mlp[1], mlp[2]) if mlp[0] == "rand"
                  else syn.body_mlp(kind, noise=mlp[2], seed=mlp[1]))
        load_mlp(net, layers)
        f = (syn.rand_feat(feat[1], 128, 128, feat[2]) if feat[0] == "rand"
             else syn.body_feat(feat[1], 128, 128, feat[2]))
        p = syn.rand_points(pts[0], pts[1], pts[2])
        ext, intr = syn.scene_camera(step)
        calib = ref_recon.pifu_calib(ext, intr, device="cpu")
        # RTL/main.py:169-183 hands netG.query a 4-stage list and uses the last one
        feats = [[torch.zeros(1, f.shape[0], 2, 2)]] * 3 + [[torch.from_numpy(f)[None]]]
        out = net.query(feats, torch.from_numpy(p)[None], calibs=calib)[0][0].numpy()
        np.savez_compressed(
            os.path.join(OUT, name + ".npz"), out=out, calib=calib.numpy(),
            meta=np.array([repr(dict(kind=kind, mlp=mlp, feat=feat, pts=pts, step=step))]))
        xyz = orthogonal(torch.from_numpy(p)[None], calib)[0].numpy()
        inside = (np.abs(xyz[0]) <= 1) & (np.abs(xyz[1]) <= 1)
        print(name, out.shape, float(out.min()), float(out.max()), "in-image:", int(inside.sum()),
              "zeros:", int((out == 0).all(0).sum()))


@torch.no_grad()
def gen_index_orthogonal_calib():
    import recon as ref_recon
    from monoport.lib.modeling.geometry import index, orthogonal
    f = syn.rand_feat(256, 128, 128, 41)
    rs = np.random.RandomState(42)
    uv = rs.uniform(-1.1, 1.1, size=(2, 256)).astype(np.float32)
    uv[:, :4] = np.array([[-1, 1, -1, 1], [-1, -1, 1, 1]], np.float32)  # exact corners
    out = index(torch.from_numpy(f)[None], torch.from_numpy(uv)[None])[0].numpy()
    np.savez_compressed(os.path.join(OUT, "index.npz"), out=out, uv=uv,
                        meta=np.array(["feat=rand_feat(256,128,128,41)"]))
    p = syn.rand_points(1000, 43, 1.0)
    ext, intr = syn.scene_camera(57)
    calib = ref_recon.pifu_calib(ext, intr, device="cpu")
    o = orthogonal(torch.from_numpy(p)[None], calib)[0].numpy()
    np.savez_compressed(os.path.join(OUT, "orthogonal.npz"), out=o, calib=calib.numpy(),
                        meta=np.array(["points=rand_points(1000,43,1.0); scene_camera(57)"]))
    steps = [0, 3, 33, 90, 181]
    calibs = []
    for s in steps:
        ext, intr = syn.scene_camera(s)
        e0, i0 = ext.copy(), intr.copy()
        calibs.append(ref_recon.pifu_calib(ext, intr, device="cpu").numpy())
        assert (e0 == ext).all() and (i0 == intr).all()
    np.savez_compressed(os.path.join(OUT, "pifu_calib.npz"), steps=np.array(steps),
                        calib=np.concatenate(calibs, 0))
    print("index", out.shape, "orthogonal", o.shape, "calib", len(steps))


@torch.no_grad()
def gen_forward_vertices():
    import recon as ref_recon
    store = {}
    for res, seed in ((33, 51), (65, 52)):
        vol = syn.blob_volume(res, seed)
        for d in ("front", "back", "left", "right"):
            x, y, z, n = ref_recon.forward_vertices(torch.from_numpy(vol)[None, None], d)
            key = "r%d_%s_" % (res, d)
            store[key + "X"] = x.numpy()
            store[key + "Y"] = y.numpy()
            store[key + "Z"] = z.numpy()
            store[key + "norm"] = n.numpy()
            print("forward_vertices", res, d, x.shape[0], "nan:", int(torch.isnan(z).sum()))
    store["meta"] = np.array(["vol=blob_volume(res,seed) for (33,51),(65,52)"])
    np.savez_compressed(os.path.join(OUT, "forward_vertices.npz"), **store)


@torch.no_grad()
def gen_forward_vertices_edges():
    """The reference's forward_vertices on the adversarial volumes of tests/surface_cases.py: hits at every border of
    the box and in the last voxel, plateaus, values exactly 0.5, zero-length normals and non-finite entries.  Only
    the results are stored; the tests rebuild the volumes from the seeds."""
    import recon as ref_recon
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import surface_cases as sc
    store = {}
    cases = [("d40_%s" % kind, sc.depth_case(40, kind)[0], sc.DIRECTIONS) for kind in sc.KINDS]
    cases.append(("nonfinite", sc.nonfinite_volume(*sc.NONFINITE), ("front", "left")))
    for name, vol, directions in cases:
        for d in directions:
            x, y, z, n = ref_recon.forward_vertices(torch.from_numpy(vol)[None, None], d)
            key = "%s_%s_" % (name, d)
            store[key + "X"] = x.numpy().astype(np.int16)  # r <= 40
            store[key + "Y"] = y.numpy().astype(np.int16)
            store[key + "Z"] = z.numpy()
            store[key + "norm"] = n.numpy()
            assert z.dtype == torch.float32 and n.dtype == torch.float32
            print("forward_vertices_edges", name, d, x.shape[0], "nan Z:", int(torch.isnan(z).sum()),
                  "nan normal rows:", int(torch.isnan(n).any(1).sum()))
    store["meta"] = np.array(["surface_cases.depth_case(40, kind) for smooth/binary/quant, four directions; "
                              "surface_cases.nonfinite_volume(*NONFINITE), front and left; X, Y as int16"])
    path = os.path.join(OUT, "forward_vertices_edges.npz")
    np.savez_compressed(path, **store)
    print("forward_vertices_edges.npz: %d bytes" % os.path.getsize(path))


@torch.no_grad()
def gen_colorization():
    """RTL/main.py:201-249 driven with the reference's orthogonal + netC.query + recon."""
    import recon as ref_recon
    from monoport.lib.modeling.geometry import orthogonal
    res = 33
    net = ref_net("C")
    load_mlp(net, syn.rand_mlp("C", 61, 2.0))
    f = syn.rand_feat(512, 128, 128, 62)
    feats = [[torch.from_numpy(f)[None]]]
    vol = syn.blob_volume(res, 63)
    X, Y, Z, norm = ref_recon.forward_vertices(torch.from_numpy(vol)[None, None], "front")
    ext, intr = syn.scene_camera(21)
    calib = ref_recon.pifu_calib(ext, intr, device="cpu")
    canvas = torch.ones((res, res, 3), dtype=torch.float32)
    b_min = torch.tensor([-1.0, -1.0, -1.0])
    b_max = torch.tensor([1.0, 1.0, 1.0])
    mat = torch.eye(4, dtype=torch.float32)
    length = b_max - b_min
    for i in range(3):
        mat[i, i] = length[i] / res
    mat[0:3, 3] = b_min
    # normal mode (main.py:219-225)
    img_n = canvas.clone()
    img_n[X, Y, :] = ((norm + 1) / 2).clamp(0, 1)
    # texture mode (main.py:228-248)
    verts = torch.stack([X.float(), Y.float(), res - Z.float()], dim=1)
    samples = verts.unsqueeze(0).permute(0, 2, 1)
    samples = orthogonal(samples, mat.unsqueeze(0))
    preds = net.query(feats, points=samples, calibs=calib)[0]
    color = (preds[0] * 0.5 + 0.5).t()
    img_t = canvas.clone()
    img_t[X, Y, :] = color
    np.savez_compressed(os.path.join(OUT, "colorization.npz"), norm_image=img_n.numpy(),
                        tex_image=img_t.numpy(), calib=calib.numpy(),
                        meta=np.array(["res=33 netC=rand_mlp(C,61,2.0) feat=rand_feat(512,128,128,62) "
                                       "vol=blob_volume(33,63) scene_camera(21)"]))
    print("colorization", int(X.shape[0]), "verts")


@torch.no_grad()
def gen_encoders():
    """netG.filter / netC.filter (MonoPortNet.py:31-46) under seeded weights; stores a strided
    slice of every output (the full maps are 16-33 MB)."""
    store = {}
    netg, netc = ref_net("G"), ref_net("C")
    for name, net in (("G", netg), ("C", netc)):
        shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
        sd = syn.seeded_state_dict(shapes, 71 if name == "G" else 72)
        net.image_filter.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    img = torch.from_numpy(syn.synthetic_image(73))[None]
    feats_g = netg.filter(img)
    feats_c = netc.filter(img, feat_prior=feats_g[-1][-1])
    assert len(feats_g) == 4 and len(feats_c) == 1
    for i, st in enumerate(feats_g):
        store["G%d" % i] = st[0][0, ::8, ::8, ::8].numpy()
        store["G%d_stats" % i] = np.array([st[0].mean().item(), st[0].std().item()], np.float64)
    store["C0"] = feats_c[0][0][0, ::8, ::8, ::8].numpy()
    store["C0_stats"] = np.array([feats_c[0][0].mean().item(), feats_c[0][0].std().item()])
    # full-resolution coverage of the maps the query kernels read (the strided slice sees 1 element in
    # 512): every element of G3 / C0 enters the mean of its 8 x 8 pixel block (per channel) and the
    # mean over channels of its pixel, so a wrong convolution tile cannot hide between the samples
    for key, t in (("G3", feats_g[-1][0][0]), ("C0", feats_c[0][0][0])):
        c, hh, ww = t.shape
        store[key + "_block8"] = t.reshape(c, hh // 8, 8, ww // 8, 8).double().mean((2, 4)).float().numpy()
        store[key + "_pixel"] = t.double().mean(0).float().numpy()
    store["meta"] = np.array(["img=synthetic_image(73); seeds 71 (G) / 72 (C); slice [::8,::8,::8]; "
                              "*_block8 = per-channel means of 8x8 pixel blocks, *_pixel = channel means"])
    np.savez_compressed(os.path.join(OUT, "encoders.npz"), **store)
    print("encoders", store["G3"].shape, store["C0"].shape, store["G3_stats"], store["C0_stats"])


@torch.no_grad()
def gen_pipeline():
    """The per-frame call sequence of RTL/main.py:389-428 with the reference's netG.query as
    query_func; the octree driver is OUR restatement (implicit_seg is not vendored)."""
    import recon as ref_recon
    from oracle import pifu_oracle as orc
    net = ref_net("G")
    load_mlp(net, syn.body_mlp("G", noise=0.05, seed=81))
    f = syn.body_feat(256, 128, 128, 82)
    feats = [[torch.zeros(1, 256, 2, 2)]] * 3 + [[torch.from_numpy(f)[None]]]
    ext, intr = syn.scene_camera(24)
    calib = ref_recon.pifu_calib(ext, intr, device="cpu")

    def query_func(points):  # RTL/main.py:169-183 on [3,N] numpy
        p = torch.from_numpy(points.T.copy())[None]          # [1,N,3]
        samples = p.repeat(1, 1, 1).permute(0, 2, 1)        # [1,3,N]
        return net.query(feats, points=samples, calibs=calib)[0][0, 0].numpy()

    res = [9, 17, 33]
    stats = []
    sdf = orc.seg3d_lossless(query_func, [-1, -1, -1], [1, 1, 1], res, stats=stats)
    X, Y, Z, norm = ref_recon.forward_vertices(torch.from_numpy(sdf)[None, None], "front")
    img = torch.ones((res[-1], res[-1], 3))
    img[X, Y, :] = ((norm + 1) / 2).clamp(0, 1)
    np.savez_compressed(os.path.join(OUT, "pipeline.npz"), sdf=sdf, X=X.numpy(), Y=Y.numpy(),
                        Z=Z.numpy(), norm=norm.numpy(), render_norm=img.numpy(),
                        stats=np.array(stats), calib=calib.numpy(),
                        meta=np.array(["mlp=body_mlp(G,noise=.05,seed=81) feat=body_feat(256,128,128,82) "
                                       "scene_camera(24) res=[9,17,33]"]))
    print("pipeline", stats, int(X.shape[0]), "verts; margin", float(np.abs(sdf - 0.5).min()))


def dense_lattice(res):
    """p = ((i + 0.5) / res) * 2 - 1 for i in [0, res)^3, ordered
    [z, y, x] (x fastest) -> [3, res^3] f32."""
    g = ((np.arange(res, dtype=np.float32) + np.float32(0.5)) / np.float32(res)) * np.float32(2) - np.float32(1)
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([xx.reshape(-1), yy.reshape(-1), zz.reshape(-1)], 0).astype(np.float32)


@torch.no_grad()
def gen_dense64():
    """BASELINE configs[0]: the dense 64^3 grid (262,144 points) through the REFERENCE netG.query
    on the CPU, no octree.  Three cases: F-rand head on a seeded feature map, F-body head on the
    body feature map (the HIP kernel sees bit-identical features: 1e-4 bar), and the F-rand head
    on the output of the REFERENCE encoder netG.filter(image) (the GPU test runs OUR encoder on
    the GPU: encoder-in-the-loop error, reported)."""
    import time
    import recon as ref_recon
    res = 64
    p = torch.from_numpy(dense_lattice(res))[None]
    ext, intr = syn.scene_camera(30)
    calib = ref_recon.pifu_calib(ext, intr, device="cpu")
    store = {"calib": calib.numpy()}
    times = {}
    net = ref_net("G")
    load_mlp(net, syn.rand_mlp("G", 91, 2.0))
    f = syn.rand_feat(256, 128, 128, 92)
    feats = [[torch.zeros(1, 256, 2, 2)]] * 3 + [[torch.from_numpy(f)[None]]]
    t0 = time.perf_counter()
    store["out_rand"] = net.query(feats, p, calibs=calib)[0][0, 0].numpy()
    times["query_dense64_s"] = time.perf_counter() - t0
    # encoder in the loop: seeded encoder weights (71), synthetic image 74, F-rand head
    shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
    sd = syn.seeded_state_dict(shapes, 71)
    net.image_filter.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    img = torch.from_numpy(syn.synthetic_image(74))[None]
    t0 = time.perf_counter()
    feats_enc = net.filter(img)
    times["filter_s"] = time.perf_counter() - t0
    store["out_enc"] = net.query(feats_enc, p, calibs=calib)[0][0, 0].numpy()
    store["enc_feat_slice"] = feats_enc[-1][0][0, ::8, ::8, ::8].numpy()
    load_mlp(net, syn.body_mlp("G", noise=0.05, seed=93))
    fb = syn.body_feat(256, 128, 128, 94)
    feats = [[torch.zeros(1, 256, 2, 2)]] * 3 + [[torch.from_numpy(fb)[None]]]
    store["out_body"] = net.query(feats, p, calibs=calib)[0][0, 0].numpy()
    store["meta"] = np.array([
        "lattice=dense_lattice(64) scene_camera(30); out_rand: rand_mlp(G,91,2.0) rand_feat(256,128,128,92); "
        "out_body: body_mlp(G,.05,93) body_feat(256,128,128,94); out_enc: rand_mlp(G,91,2.0) on "
        "reference netG.filter(synthetic_image(74)), encoder seeded_state_dict(.,71); "
        "reference CPU times here (%d threads): %r" % (torch.get_num_threads(), times)])
    np.savez_compressed(os.path.join(OUT, "dense64.npz"), **store)
    for k in ("out_rand", "out_enc", "out_body"):
        o = store[k]
        print("dense64", k, o.shape, float(o.min()), float(o.max()), "zeros:", int((o == 0).sum()))
    print("dense64 times", times)


# BASELINE configs[1]-size fixtures: name -> (head, feature seed, camera step).  "pipeline257" keeps
# round 2's scene (its camera was picked for the widest gap between a queried value and 0.5); the two
# round-3 scenes were NOT picked: their margins are recorded in the fixture, and the tests compare
# node sets modulo the neighbourhood of nodes whose reference value is within fp32 noise of 0.5.
# "soft": k = 6 and noise 1.0 -- a wide, unsaturated transition band in which every weight of the
# head and every feature channel moves the occupancy.
PIPE257_SCENES = {
    "pipeline257": (dict(k=40.0, c=2.0, noise=0.05, seed=95), 96, 170),
    "pipeline257_b": (dict(k=40.0, c=2.0, noise=0.05, seed=195), 196, 40),
    "pipeline257_soft": (dict(k=6.0, c=2.0, noise=1.0, seed=295), 296, 250),
}
# BASELINE configs[4] size: the body / camera the 513^3 GPU tests reconstruct (tests/test_recon_gpu.py:
# test_config5_513_fp16_weights), 17..513 through the reference's netG.query -- so that the config has a
# reference-produced value behind every node it queries, f32 and f16-weight kernels alike.
PIPE513_SCENES = {
    "pipeline513": (dict(k=40.0, c=2.0, noise=0.05, seed=1), 2, 30),
    # the same sharp body under a head whose seeded weights are 40x larger (noise 2.0, other seed / map /
    # camera): rounding the weights of layers 0-3 to f16 moves the occupancy by up to ~1e-4 here (1e-7 in the
    # scene above, whose weights that matter -- 40, 31.25, 1 -- are exact in f16), so the fp16-weight kernel
    # of configs[4] is held to its 3e-4 on a field that notices
    "pipeline513_w": (dict(k=40.0, c=2.0, noise=2.0, seed=501), 502, 70),
}


@torch.no_grad()
def gen_pipeline257(name="pipeline257", res=(17, 33, 65, 129, 257)):
    """BASELINE configs[1] size (configs[4] size with res = 17..513, gen_pipeline513): one frame with the REFERENCE netG.query as query_func
    (RTL/main.py:169-183) and the reference forward_vertices; the octree schedule is OUR
    restatement (implicit_seg is not vendored).  Stored: the set of nodes the octree queried
    (bit mask over the 257^3 lattice) with the reference's value at each of them in raster
    order, per-level counts, X / Y / Z / norm of the front view, and the smallest |value - 0.5|."""
    import time
    import recon as ref_recon
    from oracle import pifu_oracle as orc
    head, feat_seed, step = {**PIPE257_SCENES, **PIPE513_SCENES}[name]
    net = ref_net("G")
    load_mlp(net, syn.body_mlp("G", **head))
    f = syn.body_feat(256, 128, 128, feat_seed)
    feats = [[torch.zeros(1, 256, 2, 2)]] * 3 + [[torch.from_numpy(f)[None]]]
    ext, intr = syn.scene_camera(step)
    calib = ref_recon.pifu_calib(ext, intr, device="cpu")
    res = list(res)
    rf = res[-1]
    queried = np.zeros((rf, rf, rf), bool)

    def query_func(points):  # RTL/main.py:169-183 on [3,N] numpy
        pt = torch.from_numpy(points.T.copy())[None]          # [1,N,3]
        samples = pt.repeat(1, 1, 1).permute(0, 2, 1)        # [1,3,N]
        return net.query(feats, points=samples, calibs=calib)[0][0, 0].numpy()

    stats = []
    t0 = time.perf_counter()
    sdf = orc.seg3d_lossless(query_func, [-1, -1, -1], [1, 1, 1], res, stats=stats,
                             evaluated_out=queried)
    t1 = time.perf_counter()
    X, Y, Z, norm = ref_recon.forward_vertices(torch.from_numpy(sdf)[None, None], "front")
    t2 = time.perf_counter()
    assert int(queried.sum()) == sum(stats)
    vals = sdf[queried]
    margin = float(np.abs(vals - 0.5).min())
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), queried=np.packbits(queried.reshape(-1)),
        values=vals.astype(np.float32), stats=np.array(stats), X=X.numpy().astype(np.int16),
        Y=Y.numpy().astype(np.int16), Z=Z.numpy(), norm=norm.numpy(), calib=calib.numpy(),
        margin=np.float64(margin),
        meta=np.array(["mlp=body_mlp(G,%r) feat=body_feat(256,128,128,%d) scene_camera(%d) "
                       "res=17..%d; reference CPU times (%d threads): octree+query %.2fs, "
                       "forward_vertices %.2fs" % (head, feat_seed, step, rf, torch.get_num_threads(), t1 - t0,
                                                   t2 - t1)]))
    sat = float(((vals == 0) | (vals >= 1)).mean())
    print(name, stats, sum(stats), int(X.shape[0]), "verts; margin %.3g; saturated values %.1f%%; "
          "values in (0.01, 0.99): %.1f%%; octree+query %.2fs forward_vertices %.2fs"
          % (margin, 100 * sat, 100 * float(((vals > 0.01) & (vals < 0.99)).mean()), t1 - t0, t2 - t1))


# BASELINE configs[2]: both encoders in the loop (RTL/main.py:366-379), geometry + per-vertex colour.
COLOR257 = dict(img_g=75, img_c=76, enc_g=71, enc_c=72, head_g=dict(k=40.0, c=2.0, noise=0.05, seed=395),
                thick=0.12, head_c=("rand", 77, 0.6), step=115)


@torch.no_grad()
def gen_pipeline257_color(name="pipeline257_color"):
    """BASELINE configs[2] end to end through the REFERENCE's modules: image -> netG.filter ->
    netC.filter(image_c, feat_prior=feat_G[-1][-1]) (RTL/main.py:366-379) -> the 17..257 octree with the
    reference's netG.query as query_func (:169-183; the schedule is OUR restatement, implicit_seg is
    not vendored) -> the reference's forward_vertices (:401-406) -> the texture branch of
    ``colorization`` (:228-248) with the reference's orthogonal and netC.query.

    The netG head is synthetic.readout_body_mlp: a slab whose half thickness is a linear readout of
    the 256 ENCODER channels, fitted here to the reference encoder's output so that it is positive
    inside the silhouette of the input image.  The readout vector is an INPUT of the scene that only
    the reference can produce; it is stored in the fixture next to the reference's outputs."""
    import time
    import recon as ref_recon
    from monoport.lib.modeling.geometry import orthogonal
    from oracle import pifu_oracle as orc
    cfg = COLOR257
    netg, netc = ref_net("G"), ref_net("C")
    for net, seed in ((netg, cfg["enc_g"]), (netc, cfg["enc_c"])):
        shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
        net.image_filter.load_state_dict(
            {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(shapes, seed).items()})
    img_g = torch.from_numpy(syn.synthetic_image(cfg["img_g"]))[None]
    img_c = torch.from_numpy(syn.synthetic_image(cfg["img_c"]))[None]
    t0 = time.perf_counter()
    feats_g = netg.filter(img_g)                                   # RTL/main.py:366-369
    t1 = time.perf_counter()
    feats_c = netc.filter(img_c, feat_prior=feats_g[-1][-1])       # :372-379
    t2 = time.perf_counter()
    # the readout: channels weighted by how well they separate the silhouette from the background
    f = feats_g[-1][0][0].numpy().astype(np.float64)
    zf, _ = syn.body_depth_maps(128, 128)
    inside = zf > -3
    d = (f[:, inside].mean(1) - f[:, ~inside].mean(1)) / (f[:, inside].std(1) + f[:, ~inside].std(1) + 1e-9)
    readout = (d / np.abs(d).sum()).astype(np.float32)
    r = np.tensordot(readout.astype(np.float64), f, 1)
    r0 = float(np.float32(0.5 * (r[inside].mean() + r[~inside].mean())))
    thick = float(np.float32(cfg["thick"] / (r[inside].mean() - r0)))
    load_mlp(netg, syn.readout_body_mlp(readout, r0, thick, **cfg["head_g"]))
    load_mlp(netc, syn.rand_mlp("C", cfg["head_c"][1], cfg["head_c"][2]))
    ext, intr = syn.scene_camera(cfg["step"])
    calib = ref_recon.pifu_calib(ext, intr, device="cpu")
    res = [17, 33, 65, 129, 257]
    rf = res[-1]
    queried = np.zeros((rf, rf, rf), bool)

    ns = main_py_namespace()
    ns["netG"] = netg

    def query_func(points):  # the reference's OWN query_func (RTL/main.py:169-183, compiled from the file) on [3,N] numpy
        pt = torch.from_numpy(points.T.copy())[None]          # [1,N,3], what Seg3dLossless hands it
        return ns["query_func"](pt, feats_g, calib)[0, 0].numpy()

    stats = []
    t3 = time.perf_counter()
    sdf = orc.seg3d_lossless(query_func, [-1, -1, -1], [1, 1, 1], res, stats=stats, evaluated_out=queried)
    t4 = time.perf_counter()
    X, Y, Z, norm = ref_recon.forward_vertices(torch.from_numpy(sdf)[None, None], "front")
    t5 = time.perf_counter()
    # RTL/main.py:201-210, :228-248
    canvas = torch.ones((rf, rf, 3), dtype=torch.float32)
    b_min, b_max = torch.tensor([-1.0, -1.0, -1.0]), torch.tensor([1.0, 1.0, 1.0])
    mat = torch.eye(4, dtype=torch.float32)
    length = b_max - b_min
    for i in range(3):
        mat[i, i] = length[i] / rf
    mat[0:3, 3] = b_min
    verts = torch.stack([X.float(), Y.float(), rf - Z.float()], dim=1)
    samples = verts.unsqueeze(0).repeat(1, 1, 1).permute(0, 2, 1)
    samples = orthogonal(samples, mat.unsqueeze(0))
    preds = netc.query(feats_c, points=samples, calibs=calib)[0]
    color = (preds[0] * 0.5 + 0.5).t()
    t6 = time.perf_counter()
    image = canvas.clone()
    image[X, Y, :] = color
    img_n = canvas.clone()
    img_n[X, Y, :] = ((norm + 1) / 2).clamp(0, 1)
    vals = sdf[queried]
    margin = float(np.abs(vals - 0.5).min())
    times = dict(filter_g=t1 - t0, filter_c=t2 - t1, octree_query=t4 - t3, forward_vertices=t5 - t4,
                 color_query=t6 - t5)
    np.savez_compressed(
        os.path.join(OUT, name + ".npz"), queried=np.packbits(queried.reshape(-1)),
        values=vals.astype(np.float32), stats=np.array(stats), X=X.numpy().astype(np.int16),
        Y=Y.numpy().astype(np.int16), Z=Z.numpy(), norm=norm.numpy(), color=color.numpy(),
        tex_image=image.numpy(), norm_image=img_n.numpy(), calib=calib.numpy(), readout=readout,
        r0=np.float32(r0), thick=np.float32(thick), margin=np.float64(margin),
        featG_slice=feats_g[-1][0][0, ::8, ::8, ::8].numpy(), featC_slice=feats_c[0][0][0, ::8, ::8, ::8].numpy(),
        meta=np.array(["COLOR257=%r; reference CPU times (%d threads): %r" % (cfg, torch.get_num_threads(), times)]))
    print(name, stats, sum(stats), int(X.shape[0]), "verts; margin %.3g; readout inside %.3f outside %.3f r0 %.3f "
          "thick %.4f; colour range [%.3f, %.3f]; times %r"
          % (margin, r[inside].mean(), r[~inside].mean(), r0, thick, float(color.min()), float(color.max()), times))


def main_py_namespace(device="cpu"):
    """RTL/main.py cannot be imported (cv2, flask, GL, streamer, human_inst_seg, implicit_seg at module scope), but
    its hot-path code is plain torch: this EXECUTES the reference's own source for those pieces -- nothing is
    restated -- by parsing the file and compiling, unchanged, the module-level statements that set up the colour
    variables (:185-210, minus the Seg3dLossless construction), the functions ``query_func`` (:169-183; it reads
    the global ``netG``: set ``ns["netG"]``), ``colorization`` (:212-249) and
    ``visulization`` (:252-281), and the two "update input by removing bg" lambdas of the processors list
    (:352-364, found by the dict key they produce).  Returns the namespace; ``ns["lambda_input_netG"]`` /
    ``ns["lambda_input_netC"]`` are the lambdas."""
    import ast
    import torch.nn.functional as F
    from monoport.lib.modeling.geometry import orthogonal
    path = os.path.join(REF, "RTL", "main.py")
    src = open(path).read()
    tree = ast.parse(src, path)
    want_funcs = {"colorization", "visulization", "query_func"}
    want_names = {"b_min", "b_max", "resolutions", "canvas", "mat", "length", "mat_color"}
    body = []
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in want_funcs:
            body.append(node)
        elif isinstance(node, ast.Assign):
            t = node.targets[0]
            name = t.id if isinstance(t, ast.Name) else t.value.id if isinstance(t, ast.Subscript) and isinstance(t.value, ast.Name) else None
            if name in want_names:
                body.append(node)
    assert sum(isinstance(n, ast.FunctionDef) for n in body) == 3 and len(body) >= 3 + 9, len(body)
    ns = {"torch": torch, "np": np, "F": F, "orthogonal": orthogonal, "cuda_color": device,
          "mean": torch.tensor([0.5, 0.5, 0.5]).view(1, 3, 1, 1),   # cfg.netG.mean / .std (config.py:30-31), main.py:288-289
          "std": torch.tensor([0.5, 0.5, 0.5]).view(1, 3, 1, 1)}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Lambda) and isinstance(node.body, ast.Dict):
            for k in node.body.keys:
                if isinstance(k, ast.Constant) and k.value in ("input_netG", "input_netC"):
                    found[k.value] = node
    assert set(found) == {"input_netG", "input_netC"}
    for key, node in found.items():
        ns["lambda_" + key] = eval(compile(ast.Expression(body=node), path, "eval"), ns)
    return ns


@torch.no_grad()
def gen_main_py():
    """SURVEY 8f row N3 and the colour closure pinned to the reference's OWN SOURCE (main_py_namespace): the two
    input-preparation lambdas on a seeded segmentation output, ``visulization`` on the two 257^2 renders of the
    configs[2] scene and on a seeded 129^2 render, and ``colorization`` (normal and texture branch, its own canvas
    / mat_color globals) on that scene's vertices -- which must reproduce the renders gen_pipeline257_color built
    from the same pieces by hand."""
    ns = main_py_namespace()
    store = {}
    # --- RTL/main.py:352-364
    rs = np.random.RandomState(101)
    segm = rs.uniform(-1, 1, size=(1, 4, 64, 64)).astype(np.float32)
    soft = rs.uniform(0, 1, size=(64, 64)).astype(np.float32)
    segm[0, 3] = np.where(rs.uniform(size=(64, 64)) > 0.4, soft, 0).astype(np.float32)
    segm[0, 3, :8] = 1.0
    d = {"segm": torch.from_numpy(segm)}
    for tag, (m, sd) in {"cfg": ([0.5, 0.5, 0.5], [0.5, 0.5, 0.5]), "imagenet": ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])}.items():
        ns["mean"] = torch.tensor(m).view(1, 3, 1, 1)
        ns["std"] = torch.tensor(sd).view(1, 3, 1, 1)
        store["input_netG_" + tag] = ns["lambda_input_netG"](d)["input_netG"].numpy()
    store["input_netC"] = ns["lambda_input_netC"](d)["input_netC"].numpy()
    # --- RTL/main.py:212-249 on the configs[2] scene (needs tests/golden/pipeline257_color.npz)
    g = np.load(os.path.join(OUT, "pipeline257_color.npz"))
    cfg = COLOR257
    netg, netc = ref_net("G"), ref_net("C")
    for net, seed in ((netg, cfg["enc_g"]), (netc, cfg["enc_c"])):
        shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
        net.image_filter.load_state_dict(
            {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(shapes, seed).items()})
    load_mlp(netc, syn.rand_mlp("C", cfg["head_c"][1], cfg["head_c"][2]))
    img_g = torch.from_numpy(syn.synthetic_image(cfg["img_g"]))[None]
    img_c = torch.from_numpy(syn.synthetic_image(cfg["img_c"]))[None]
    feats_c = netc.filter(img_c, feat_prior=netg.filter(img_g)[-1][-1])
    X = torch.from_numpy(g["X"].astype(np.int64))
    Y = torch.from_numpy(g["Y"].astype(np.int64))
    Z, norm, calib = torch.from_numpy(g["Z"]), torch.from_numpy(g["norm"]), torch.from_numpy(g["calib"])
    assert ns["resolutions"][-1] == 257 and tuple(ns["canvas"].shape) == (257, 257, 3)
    render_norm = ns["colorization"](netc, None, X, Y, Z, calib, norm)
    render_tex = ns["colorization"](netc, feats_c, X, Y, Z, calib, None)
    assert ns["colorization"](netc, feats_c, None, None, None, calib) is None
    same_n = bool(np.array_equal(render_norm.numpy(), g["norm_image"]))
    same_t = float(np.abs(render_tex.numpy() - g["tex_image"]).max())
    assert same_n and same_t == 0.0, (same_n, same_t)  # the hand-assembled renders of the fixture ARE the closure's
    # --- RTL/main.py:252-281
    vn, vt, vm = ns["visulization"](render_norm, render_tex)
    store["vis_norm"], store["vis_tex"], store["vis_mask"] = vn, vt, vm
    n2, t2, m2 = ns["visulization"](render_norm, None)
    assert t2 is None and np.array_equal(n2, vn)
    assert ns["visulization"](None, None) == (None, None, None)
    small = np.ones((129, 129, 3), np.float32)
    idx = rs.randint(0, 129, size=(3000, 2))
    small[idx[:, 0], idx[:, 1]] = rs.rand(3000, 3).astype(np.float32)
    s_n, _, s_m = ns["visulization"](torch.from_numpy(small), None)
    store["vis129_in"], store["vis129_norm"], store["vis129_mask"] = small, s_n, s_m
    store["meta"] = np.array(["RTL/main.py executed from source (oracle/gen_golden.py: main_py_namespace): lambdas "
                              ":352-364 on segm = RandomState(101) [1,4,64,64]; colorization :212-249 on the vertices of "
                              "pipeline257_color.npz reproduces its norm_image / tex_image exactly; visulization :252-281 of "
                              "those two renders and of a seeded 129^2 render"])
    np.savez_compressed(os.path.join(OUT, "main_py.npz"), segm=segm, **store)
    print("main_py: lambdas", store["input_netG_cfg"].shape, "visulization", vn.shape, vt.shape, int(vm.sum()),
          "foreground pixels; colorization == fixture renders:", same_n, same_t)




def gen_obj():
    """The reference's OBJ writers (monoport/lib/mesh_util.py:223-242) on the seeded mesh: the files'
    sha256 + sizes + first lines are the fixture."""
    import hashlib
    import tempfile
    from monoport.lib import mesh_util as ref_mesh
    v, f, c = syn.obj_mesh_inputs()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for key, call in (("plain", lambda p: ref_mesh.save_obj_mesh(p, v, f)),
                          ("color", lambda p: ref_mesh.save_obj_mesh_with_color(p, v, f, c))):
            path = os.path.join(d, key + ".obj")
            call(path)
            data = open(path, "rb").read()
            out[key + "_sha256"] = np.frombuffer(hashlib.sha256(data).digest(), np.uint8).copy()
            out[key + "_size"] = np.int64(len(data))
            out[key + "_head"] = np.frombuffer(data[:400], np.uint8).copy()
    np.savez_compressed(os.path.join(OUT, "obj_format.npz"), **out)
    print("obj_format", int(out["plain_size"]), int(out["color_size"]))


@torch.no_grad()
def gen_rect():
    """Non-square feature maps (tests/rect_cases.py): the reference's geometry.index on the 48 x 80, 80 x 48, two-row,
    two-column, one-row and one-column maps, and PIFuNetG / PIFuNetC.query (orthogonal under the scene camera and
    the identity, one perspective case) on 4096 points each.  Outputs and calibrations only, in one file; the
    tests rebuild maps, heads, uv and points from the seeds of the case table."""
    import recon as ref_recon
    from monoport.lib.modeling.geometry import index, orthogonal, perspective
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import rect_cases as rc
    store = {}
    for name in rc.INDEX_CASES:
        f, uv = rc.index_inputs(name)
        store[name] = index(torch.from_numpy(f)[None], torch.from_numpy(uv)[None])[0].numpy()
        print("rect", name, f.shape, store[name].shape)
    for name, case in rc.QUERY_CASES.items():
        kind, layers, f, p = rc.query_inputs(name)
        net = ref_net(kind)
        load_mlp(net, layers)
        if case["camera"] == "scene":
            calib = ref_recon.pifu_calib(*syn.scene_camera(rc.SCENE_STEP), device="cpu")
        elif case["camera"] == "eye":
            calib = torch.eye(4)[None]
        else:
            calib = torch.from_numpy(rc.persp_calib())
            net.projection = perspective  # opt_net.projection = "perspective" (MonoPortNet.py:27)
        feats = [[torch.zeros(1, f.shape[0], 2, 2)]] * 3 + [[torch.from_numpy(f)[None]]]
        out = net.query(feats, torch.from_numpy(p)[None], calibs=calib)[0][0].numpy()
        xyz = (perspective if case["camera"] == "persp" else orthogonal)(torch.from_numpy(p)[None], calib)[0].numpy()
        inside, outside = rc.inside_image(xyz), rc.outside_image(xyz)
        nan = np.isnan(out).all(0)
        assert inside.sum() >= rc.MIN_INSIDE and outside.sum() >= rc.MIN_OUTSIDE, (name, inside.sum(), outside.sum())
        assert (out[:, outside] == 0).all()
        if case["camera"] == "persp":
            at = rc.PERSP_AT
            assert nan[at:at + 4].all() and nan.sum() == 4
        else:
            assert not nan.any()
        store[name] = out
        store[name + "_calib"] = calib.numpy()
        print("rect %-14s %s map %s in-image %d outside %d NaN %d range [%.3g, %.3g]"
              % (name, out.shape, f.shape, int(inside.sum()), int(outside.sum()), int(nan.sum()),
                 float(np.nanmin(out)), float(np.nanmax(out))))
    store["meta"] = np.array(["tests/rect_cases.py: INDEX_CASES (rand_feat(256,H,W,seed), uv = RandomState(seed) in "
                              "+-1.1, corners first) and QUERY_CASES (rand_mlp(kind,seed,2.0), rand_feat(C,H,W,seed), "
                              "rect_points(H,W,seed); scene_camera(%d), identity, persp_calib())" % rc.SCENE_STEP])
    path = os.path.join(OUT, rc.FIXTURE + ".npz")
    np.savez_compressed(path, **store)
    print("%s.npz: %d bytes" % (rc.FIXTURE, os.path.getsize(path)))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ["query", "misc", "vertices", "vertices_edges", "color", "encoders", "pipeline",
                             "dense64", "obj", "pipeline257_color", "main_py", "rect"] + sorted(PIPE257_SCENES)
    if "obj" in which:
        gen_obj()
    if "query" in which:
        gen_query()
    if "misc" in which:
        gen_index_orthogonal_calib()
    if "vertices" in which:
        gen_forward_vertices()
    if "vertices_edges" in which:
        gen_forward_vertices_edges()
    if "color" in which:
        gen_colorization()
    if "encoders" in which:
        gen_encoders()
    if "pipeline" in which:
        gen_pipeline()
    if "dense64" in which:
        gen_dense64()
    for name in PIPE257_SCENES:
        if name in which:
            gen_pipeline257(name)
    for name in PIPE513_SCENES:  # not in the default list: 1.2 M points each through the reference, ~1 min
        if name in which:
            gen_pipeline257(name, res=(17, 33, 65, 129, 257, 513))
    if "pipeline257_color" in which:
        gen_pipeline257_color()
    if "main_py" in which:
        gen_main_py()
    if "rect" in which:
        gen_rect()
