"""The reference's per-frame call sequence (RTL/main.py:106-128, :169-249, :389-441) executed
against monoport_amd's drop-in modules on an MI355X and compared with the fixture the reference's
own modules produced (oracle/gen_golden.py:gen_pipeline)."""
import numpy as np
import pytest

from conftest import load_golden
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"


def _load_mlp(net, layers):
    sd = {}
    for i, (w, b) in enumerate(layers):
        sd["filters.%d.weight" % i] = torch.from_numpy(w)[:, :, None]
        sd["filters.%d.bias" % i] = torch.from_numpy(b)
    net.surface_classifier.load_state_dict(sd)


def test_main_py_call_sequence():
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.recon import colorization, forward_vertices, pifu_calib
    g = load_golden("pipeline")

    # --- model set-up as RTL/main.py:106-116
    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", noise=0.05, seed=81))
    netG.image_filter.to(DEV)
    netG.surface_classifier.to(DEV)
    netG.eval()

    # --- RTL/main.py:169-195
    def query_func(points, im_feat_list, calib_tensor):
        assert len(points) == 1
        samples = points.repeat(1, 1, 1)
        samples = samples.permute(0, 2, 1)
        return netG.query(im_feat_list, points=samples, calibs=calib_tensor)[0]

    b_min = torch.tensor([-1.0, -1.0, -1.0]).float()
    b_max = torch.tensor([1.0, 1.0, 1.0]).float()
    resolutions = [8 + 1, 16 + 1, 32 + 1]
    reconEngine = Seg3dLossless(query_func=query_func, b_min=b_min.unsqueeze(0).numpy(),
                                b_max=b_max.unsqueeze(0).numpy(), resolutions=resolutions,
                                balance_value=0.5, use_cuda_impl=False, faster=True).to(DEV)

    # --- per-frame stages, RTL/main.py:337-428
    ext, intr = syn.scene_camera(24)
    calib_tensor = pifu_calib(ext, intr, device=DEV)
    assert np.array_equal(calib_tensor.cpu().numpy(), g["calib"])
    f = torch.from_numpy(syn.body_feat(256, 128, 128, 82))[None].to(DEV)
    feat_tensor_G = [[torch.zeros(1, 256, 2, 2, device=DEV)]] * 3 + [[f]]
    sdf = reconEngine(im_feat_list=feat_tensor_G, calib_tensor=calib_tensor)
    assert sdf.shape == (1, 1, 33, 33, 33) and sdf.device.type == "cuda"
    assert list(reconEngine.last_status[1:].numpy()) == list(g["stats"])
    assert np.abs(sdf[0, 0].cpu().numpy() - g["sdf"]).max() <= 1e-4
    X, Y, Z, norm = forward_vertices(sdf, direction="front")
    assert np.array_equal(X.cpu().numpy(), g["X"]) and np.array_equal(Y.cpu().numpy(), g["Y"])
    assert np.abs(Z.cpu().numpy() - g["Z"]).max() <= 2e-3  # voxel units; sdf differs by <=1e-4
    render_norm = colorization(None, None, X, Y, Z, calib_tensor, norm, resolution=resolutions[-1])
    assert render_norm.shape == (33, 33, 3)
    assert np.abs(render_norm.cpu().numpy() - g["render_norm"]).max() <= 2e-3

    # direct query (generic path) still works next to the engine
    pts = torch.from_numpy(syn.rand_points(500, 5, 1.0).T.copy())[None].to(DEV)
    out = query_func(pts, feat_tensor_G, calib_tensor)
    assert out.shape == (1, 1, 500)


def test_empty_scene_returns_none():
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.recon import colorization, forward_vertices
    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", c=-3.0))
    netG.surface_classifier.to(DEV)
    netG.eval()
    eng = Seg3dLossless(query_func=lambda points, feats, calib: netG.query(feats, points.permute(0, 2, 1), calib)[0],
                        b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]),
                        resolutions=[9, 17], faster=True).to(DEV)
    f = torch.from_numpy(syn.body_feat(256, 128, 128, 82))[None].to(DEV)
    sdf = eng(feats=[[f]], calib=torch.eye(4, device=DEV)[None])
    assert sdf is None
    X, Y, Z, norm = forward_vertices(sdf)
    assert X is None and colorization(None, None, X, Y, Z, None, norm) is None


def test_netc_colorization_matches_reference():
    from monoport_amd.modeling import PIFuNetC
    from monoport_amd.recon import color_matrix, colorization, forward_vertices
    g = load_golden("colorization")
    res = 33
    netC = PIFuNetC()
    _load_mlp(netC, syn.rand_mlp("C", 61, 2.0))
    netC.surface_classifier.to(DEV)
    netC.eval()
    feat_C = [[torch.from_numpy(syn.rand_feat(512, 128, 128, 62))[None].to(DEV)]]
    vol = torch.from_numpy(syn.blob_volume(res, 63)).to(DEV)[None, None]
    X, Y, Z, norm = forward_vertices(vol, "front")
    calib = torch.from_numpy(g["calib"]).to(DEV)
    tex = colorization(netC, feat_C, X, Y, Z, calib, None, resolution=res,
                       mat_color=color_matrix([-1, -1, -1], [1, 1, 1], res))
    assert np.abs(tex.cpu().numpy() - g["tex_image"]).max() <= 1e-4


def test_encoder_on_gpu_close_to_reference():
    """Our encoder kernels (csrc/conv*.hip) vs the reference's CPU run of the same weights (fp32 summation order differs)."""
    from monoport_amd.modeling import PIFuNetG
    g = load_golden("encoders")
    net = PIFuNetG().eval()
    shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
    sd = syn.seeded_state_dict(shapes, 71)
    net.image_filter.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.image_filter.to(DEV)
    img = torch.from_numpy(syn.synthetic_image(73))[None].to(DEV)
    with torch.no_grad():
        fg = net.filter(img)
    for i in range(4):  # all four stacks; measured <= 6e-6 on the MI355X
        assert np.abs(fg[i][0][0, ::8, ::8, ::8].cpu().numpy() - g["G%d" % i]).max() <= 1e-4


@pytest.mark.parametrize("precision", ["f32", "f16x3"])
def test_netc_encoder_on_gpu_close_to_reference(monkeypatch, precision):
    """netC.filter (ResNet encoder + the nearest-resized, prior-first concat of MonoPortNet.py:41-45)
    on the GPU vs the reference's CPU run of the same seeded weights (fixture C0); its residual
    blocks run on csrc/conv3x3.hip (reflection padding) in either precision."""
    from monoport_amd.modeling import PIFuNetC, PIFuNetG, backbones
    monkeypatch.setattr(backbones, "ENCODER_CONV_PRECISION", precision)
    g = load_golden("encoders")
    netg, netc = PIFuNetG().eval(), PIFuNetC().eval()
    for net, seed in ((netg, 71), (netc, 72)):
        shapes = {k: tuple(v.shape) for k, v in net.image_filter.state_dict().items()}
        net.image_filter.load_state_dict(
            {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(shapes, seed).items()})
        net.image_filter.to(DEV)
    img = torch.from_numpy(syn.synthetic_image(73))[None].to(DEV)
    with torch.no_grad():
        fg = netg.filter(img)
        fc = netc.filter(img, feat_prior=fg[-1][-1])
    assert len(fc) == 1 and fc[0][0].shape == (1, 512, 128, 128)
    err = float(np.abs(fc[0][0][0, ::8, ::8, ::8].cpu().numpy() - g["C0"]).max())
    print("netC.filter (%s convs) on GPU vs reference: %.3g" % (precision, err))
    assert err <= 1e-4


def test_group_norm_and_bicubic_kernels_match_torch():
    """csrc/encoder_ops.hip against the stock PyTorch ops they replace inside the encoders."""
    from monoport_amd import ops
    torch.manual_seed(3)
    for n, c, h, w in ((1, 64, 256, 256), (1, 256, 128, 128), (3, 128, 64, 64), (2, 256, 32, 32)):
        x = (torch.randn(n, c, h, w, device=DEV) * 3 + 1.5)
        gn = torch.nn.GroupNorm(32, c).to(DEV)
        with torch.no_grad():
            gn.weight.uniform_(0.5, 1.5)
            gn.bias.uniform_(-0.5, 0.5)
            ref = gn(x)
            out = ops.group_norm(x, 32, gn.weight, gn.bias, gn.eps, relu=False)
            out_r = ops.group_norm(x, 32, gn.weight, gn.bias, gn.eps, relu=True)
        assert (out - ref).abs().max().item() <= 2e-5
        assert torch.equal(out_r, torch.relu(out))
    for n, c, h, w in ((1, 256, 64, 64), (2, 256, 32, 32), (3, 8, 5, 7)):
        x = torch.randn(n, c, h, w, device=DEV)
        skip = torch.randn(n, c, 2 * h, 2 * w, device=DEV)
        ref = torch.nn.functional.interpolate(x, scale_factor=2, mode="bicubic", align_corners=True)
        assert (ops.upsample_bicubic2x(x) - ref).abs().max().item() <= 2e-5
        assert (ops.upsample_bicubic2x(x, add=skip) - (skip + ref)).abs().max().item() <= 2e-5


def test_concat3_add_bit_exact_vs_torch():
    """The pyramid block's tail (HGFilters.py:57-60) fused: same bits as torch.cat + add."""
    from monoport_amd import ops
    g = torch.Generator().manual_seed(9)
    for n, (ca, cb, cc), hw in ((1, (128, 64, 64), (128, 128)), (3, (64, 32, 32), (8, 8)),
                               (4, (128, 64, 64), (32, 32))):
        a, b, c = (torch.randn((n, k) + hw, generator=g).to(DEV) for k in (ca, cb, cc))
        sc = torch.randn((n, ca + cb + cc) + hw, generator=g).to(DEV)
        assert ops.concat3_add_supported(a, b, c, sc)
        assert torch.equal(ops.concat3_add(a, b, c, sc), torch.cat((a, b, c), 1) + sc)
    odd = torch.randn((1, 4, 3, 3)).to(DEV)  # HW % 4 != 0 -> the modules fall back to torch ops
    assert not ops.concat3_add_supported(odd, odd, odd, torch.cat((odd, odd, odd), 1))


def test_processors_list_through_stage_pipeline():
    """The hot-path stages of RTL/main.py:326-452 as a processors=[...] list on the torch-2.x
    stage pipeline (thread + HIP stream per stage): results must equal sequential execution."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.recon import colorization, forward_vertices, pifu_calib
    from monoport_amd.stage_pipeline import StagePipeline

    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", noise=0.05, seed=81))
    shapes = {k: tuple(v.shape) for k, v in netG.image_filter.state_dict().items()}
    netG.image_filter.load_state_dict(
        {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(shapes, 71).items()})
    netG.to(DEV).eval()
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(DEV)

    def query_func(points, im_feat_list, calib_tensor):
        return netG.query(im_feat_list, points=points.permute(0, 2, 1), calibs=calib_tensor)[0]

    res = [9, 17, 33, 65]
    reconEngine = Seg3dLossless(query_func=query_func, b_min=np.array([[-1., -1., -1.]]),
                                b_max=np.array([[1., 1., 1.]]), resolutions=res, faster=True).to(DEV)
    mean, std = 0.5, 0.5
    step = [0]

    def update_camera():
        ext, intr = syn.scene_camera(step[0])
        step[0] += 3
        return ext, intr

    def filt(d):
        feats = netG.filter(d["input_netG"])
        feats[-1][0][0, 0:2].copy_(planes)  # synthetic body planes (see bench.py)
        return {**d, "feat_tensor_G": feats}

    processors = [
        lambda data: {"input": data.to(DEV, non_blocking=True)},                      # main.py:327
        lambda d: {**d, **dict(zip(["extrinsic", "intrinsic"], update_camera()))},      # :330-336
        lambda d: {**d, "calib_tensor": pifu_calib(d["extrinsic"], d["intrinsic"], device=DEV)},
        lambda d: {**d, "input_netG": (((d["input"][:, 0:3] * 0.5 + 0.5) - mean) / std)
                   * d["input"][:, 3:4]},                                             # :353-357
        filt,                                                                          # :367-370
        lambda d: {**d, "sdf": reconEngine(im_feat_list=d["feat_tensor_G"],
                                           calib_tensor=d["calib_tensor"])},           # :390-395
        lambda d: {**d, **dict(zip(["X", "Y", "Z", "norm"],
                                   forward_vertices(d["sdf"], direction="front")))},   # :401-406
        lambda d: {**d, "render_norm": colorization(None, None, d["X"], d["Y"], d["Z"],
                                                    d["calib_tensor"], d["norm"],
                                                    resolution=res[-1])},              # :418-428
    ]
    frames = []
    for i in range(5):
        img = torch.from_numpy(syn.synthetic_image(i))
        mask = (img.abs().sum(0, keepdim=True) > 0).float()
        frames.append(torch.cat([img, mask], 0)[None])

    step[0] = 0
    sequential = []
    for f in frames:
        d = f
        for p in processors:
            d = p(d)
        sequential.append(d)
    torch.cuda.synchronize()
    step[0] = 0
    piped = list(StagePipeline(frames, processors, device=DEV, max_in_flight=2))
    torch.cuda.synchronize()
    assert len(piped) == len(sequential) == 5
    for a, b in zip(piped, sequential):
        assert torch.equal(a["calib_tensor"], b["calib_tensor"])
        assert torch.equal(a["sdf"], b["sdf"])
        assert torch.equal(a["X"], b["X"]) and torch.equal(a["Z"], b["Z"])
        assert torch.equal(a["render_norm"], b["render_norm"])
    assert piped[0]["X"].shape[0] > 100


def test_visulization_matches_reference_formula():
    """RTL/main.py:252-281 restated with stock tensor ops on the CPU vs the one-pass kernel."""
    import torch.nn.functional as F
    from monoport_amd.recon import visulization
    assert visulization(None, None) == (None, None, None)
    rs = np.random.RandomState(0)
    img = np.ones((257, 257, 3), np.float32)
    idx = rs.randint(0, 257, size=(5000, 2))
    img[idx[:, 0], idx[:, 1]] = rs.rand(5000, 3).astype(np.float32)
    t = torch.from_numpy(img)
    ref = torch.rot90(t * 255.0, 1, [0, 1]).permute(2, 0, 1).unsqueeze(0)
    ref = F.interpolate(ref, size=(256, 256))[0].numpy().transpose(1, 2, 0)
    bg = np.logical_and(np.logical_and(ref[:, :, 0] == 255, ref[:, :, 1] == 255), ref[:, :, 2] == 255)
    n, tex, mask = visulization(t.to(DEV), None)
    assert tex is None and np.array_equal(n, ref)
    assert np.array_equal(mask, ~bg.reshape(256, 256, 1))


def test_obj_export_and_vertex_colors(tmp_path):
    from monoport_amd.mesh_util import save_obj_mesh, save_obj_mesh_with_color, vertex_colors
    from monoport_amd.modeling import PIFuNetC
    from monoport_amd.recon import marching_cubes
    vol = torch.from_numpy(syn.blob_volume(33, 5)).to(DEV)
    verts, faces = marching_cubes(vol[None, None])
    netC = PIFuNetC()
    _load_mlp(netC, syn.rand_mlp("C", 61, 2.0))
    netC.surface_classifier.to(DEV)
    netC.eval()
    feat_C = [[torch.from_numpy(syn.rand_feat(512, 128, 128, 62))[None].to(DEV)]]
    colors = vertex_colors(netC, feat_C, verts, torch.eye(4, device=DEV)[None])
    assert colors.shape == verts.shape and float(colors.min()) >= 0 and float(colors.max()) <= 1
    p1, p2 = tmp_path / "m.obj", tmp_path / "mc.obj"
    save_obj_mesh(str(p1), verts, faces)
    save_obj_mesh_with_color(str(p2), verts, faces, colors)
    lines = open(p2).read().splitlines()
    nv, nf = verts.shape[0], faces.shape[0]
    assert len(lines) == nv + nf and len(open(p1).read().splitlines()) == nv + nf
    v0 = lines[0].split()
    assert v0[0] == "v" and len(v0) == 7 and abs(float(v0[1]) - float(verts[0, 0])) < 1e-4
    f0 = lines[nv].split()
    assert f0[0] == "f" and [int(a) for a in f0[1:]] == [int(a) + 1 for a in faces[0].tolist()]


@pytest.mark.parametrize("skip_table", [False, True])
def test_frame_pipeline_matches_direct_calls(skip_table):
    """FramePipeline (slots x batched encoder x hipGraph) must give, frame by frame, what the
    plain call sequence gives: identical octree decisions and renders -- on the plain query path
    and with the layer-0 tables (mp_skip_table) on both sides."""
    from monoport_amd import ops
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.pipeline import FramePipeline
    from monoport_amd.recon import pifu_calib
    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", noise=0.05, seed=81))
    shapes = {k: tuple(v.shape) for k, v in netG.image_filter.state_dict().items()}
    netG.image_filter.load_state_dict(
        {k: torch.from_numpy(v) for k, v in syn.seeded_state_dict(shapes, 71).items()})
    netG.to(DEV).eval()
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(DEV)

    def hook(feat):
        feat[:, 0:2].copy_(planes[None].expand(feat.shape[0], -1, -1, -1))

    res = [9, 17, 33, 65]
    images = [torch.from_numpy(syn.synthetic_image(i))[None].to(DEV) for i in range(6)]
    calibs = [pifu_calib(*syn.scene_camera(7 * i), device=DEV) for i in range(6)]

    # direct, one frame at a time
    direct = []
    mlp = netG.surface_classifier.packed()
    with torch.no_grad():
        for img, cal in zip(images, calibs):
            feat = netG.image_filter(img, last_only=True)[-1][0]
            hook(feat)
            fh = ops.pack_features(feat)
            table = ops.skip_table(mlp, fh) if skip_table else None
            vol, st = ops.recon(mlp, fh, cal, syn.Z_SCALE, [-1] * 3, [1] * 3, res)
            x, y, z, n, c = ops.forward_vertices_raw(vol, "front")
            direct.append((st.cpu(), ops.paint(x, y, n, 0, c, res[-1], 0.5, 0.5, 0.0, 1.0).cpu()))
            if skip_table:
                table.release()

    for batch, use_graph in ((1, False), (3, True), (4, True)):  # 4: the last batch is short (6 = 4 + 2)
        pipe = FramePipeline(netG, DEV, depth=2, batch=batch, resolutions=res, feature_hook=hook,
                             use_graph=use_graph, skip_table=skip_table)
        pipe.prepare()
        got = []
        for s0 in range(0, 6, batch):
            slot = pipe.submit(images[s0:s0 + batch], calibs[s0:s0 + batch])
            slot.wait()
            assert slot.n_active == min(batch, 6 - s0)
            for b in range(slot.n_active):
                got.append((slot.status[b].cpu(), slot.renders[b].cpu(), slot.feats_hwc[b].clone()))
        assert len(got) == 6
        for f, ((st_d, r_d), (st_p, r_p, fh_p)) in enumerate(zip(direct, got)):
            assert torch.equal(st_d, st_p)  # same points queried at every level
            # at batch > 1 the convolution launches pick other tile shapes (another summation order): features differ in the last bits
            assert (r_d - r_p).abs().max().item() <= (0.0 if batch == 1 else 2e-3)
            # given the slot's own features, everything downstream of them is the single-frame calls bit for bit
            with torch.no_grad():
                table = ops.skip_table(mlp, fh_p) if skip_table else None
                vol, st = ops.recon(mlp, fh_p, calibs[f], syn.Z_SCALE, [-1] * 3, [1] * 3, res)
                x, y, z, n, c = ops.forward_vertices_raw(vol, "front")
                r_own = ops.paint(x, y, n, 0, c, res[-1], 0.5, 0.5, 0.0, 1.0).cpu()
                if skip_table:
                    table.release()
            assert torch.equal(st.cpu(), st_p) and torch.equal(r_own, r_p)


def test_frame_pipeline_is_deterministic_under_concurrency():
    """Three slots on three streams, 4 frames each, 36 frames pushed twice without waiting in
    between: every frame's octree counts and render must come out bit-identical in both passes
    (per-stream scratch arenas, no cross-stream sharing of level buffers)."""
    import bench
    pipe = bench.make_pipeline(torch.device(DEV), 3, True, [17, 33, 65, 129], False, "f32", 4)
    from monoport_amd.recon import pifu_calib
    images = [torch.from_numpy(syn.synthetic_image(i))[None].to(DEV) for i in range(4)]
    calibs = [pifu_calib(*syn.scene_camera(5 * i), device=DEV) for i in range(36)]

    def one_pass():
        out = []
        for s0 in range(0, 36, 4):
            slot = pipe.submit([images[s % 4] for s in range(s0, s0 + 4)], calibs[s0:s0 + 4])
            with torch.cuda.stream(slot.stream):  # snapshot on the slot's stream, no host sync
                out.append((slot.status.clone(), torch.stack(slot.renders[:4]).clone()))
        pipe.synchronize()
        return out

    first, second = one_pass(), one_pass()
    for (st1, r1), (st2, r2) in zip(first, second):
        assert torch.equal(st1, st2) and torch.equal(r1, r2)
    counts = torch.stack([st for st, _ in first]).cpu()
    assert (counts[:, :, 0] == 1).all() and len(set(counts[:, :, 4].flatten().tolist())) > 10


def test_frame_pipeline_holds_a_fixed_amount_of_memory():
    """Weak #10 of the round-5 verdict: a FramePipeline (what bench.py's headline runs) must hold what it holds after
    its first round of submissions and not a byte more -- torch's reserved bytes, the C side's arenas / weights /
    arena count (mp_memory_stats) and the registered skip tables (one per frame of every slot) are identical after 3 and
    after 12 rounds over the slots (torch's allocated bytes within 1 %); closing the pipeline gives the tables back."""
    import gc
    import bench
    from monoport_amd import ops
    from monoport_amd.recon import pifu_calib
    gc.collect()
    torch.cuda.synchronize()
    base = ops.memory_stats(DEV)
    pipe = bench.make_pipeline(torch.device(DEV), 3, True, [17, 33, 65, 129, 257], False, "f32", 4)
    images = [torch.from_numpy(syn.synthetic_image(i))[None].to(DEV) for i in range(4)]
    calibs = [pifu_calib(*syn.scene_camera(7 * i), device=DEV) for i in range(12)]

    def rounds(n):
        for r in range(n):
            for s0 in range(0, 12, 4):
                pipe.submit([images[(s + r) % 4] for s in range(s0, s0 + 4)], calibs[s0:s0 + 4])
        pipe.synchronize()
        st = ops.memory_stats(DEV)
        return (torch.cuda.memory_reserved(DEV), torch.cuda.memory_allocated(DEV), st["arena_bytes"], st["weight_bytes"],
                st["arenas"], st["skip_tables"])

    try:
        after3 = rounds(3)
        after12 = rounds(9)
        print("FramePipeline 3 slots x 4 frames at 17..257: reserved %.2f GB, allocated %.2f GB, arenas %.0f MB in %d, "
              "%d tables" % (after3[0] / 2 ** 30, after3[1] / 2 ** 30, after3[2] / 2 ** 20, after3[4], after3[5]))
        # reserved bytes, arenas, weights and tables exactly; torch's ALLOCATED bytes within 1 % (whether the last
        # submissions' status / count / render tensors -- and what earlier tests of the process left to the garbage
        # collector -- have been released yet is a matter of timing: 0.2-3 MB of 3 GB seen)
        assert after12[0] == after3[0] and after12[2:] == after3[2:]
        assert abs(after12[1] - after3[1]) <= 0.01 * after3[1]
        assert after3[5] - base["skip_tables"] == 12  # one table per frame of every slot
    finally:
        pipe.close()
    del pipe
    gc.collect()
    end = ops.memory_stats(DEV)
    assert end["skip_tables"] == base["skip_tables"] and end["arena_bytes"] <= after3[2]


def test_prepare_inputs_bit_exact_vs_reference_expressions():
    """RTL/main.py:352-364: the two background-removal processors, fused; same bits as the
    reference's chain of torch ops on the same device."""
    from monoport_amd.recon import prepare_inputs
    g = torch.Generator().manual_seed(5)
    segm = torch.rand((1, 4, 512, 512), generator=g) * 2 - 1
    segm[:, 3] = (torch.rand((1, 512, 512), generator=g) > 0.4).float() * torch.rand((1, 512, 512), generator=g)
    segm = segm.to("cuda:0")
    mean_l, std_l = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    mean = torch.tensor(mean_l).to("cuda:0").view(1, 3, 1, 1)
    std = torch.tensor(std_l).to("cuda:0").view(1, 3, 1, 1)
    want_g = (((segm[:, 0:3] * 0.5 + 0.5) - mean) / std) * segm[:, 3:4]
    want_c = segm[:, 0:3] * segm[:, 3:4]
    got_g, got_c = prepare_inputs(segm, mean_l, std_l)
    assert torch.equal(got_g, want_g) and torch.equal(got_c, want_c)
    only_g, none_c = prepare_inputs(segm, mean_l, std_l, with_color=False)
    assert none_c is None and torch.equal(only_g, want_g)


def test_pre_and_post_steps_vs_the_references_own_source():
    """SURVEY 8f row N3 against REFERENCE OUTPUT: tests/golden/main_py.npz holds what RTL/main.py's own source
    produces -- its two input-preparation lambdas (:352-364), ``visulization`` (:252-281) and ``colorization``
    (:212-249), compiled unchanged out of the file by oracle/gen_golden.py: main_py_namespace (the module itself
    cannot be imported) -- for a seeded segmentation output and for the renders of the configs[2] scene."""
    from monoport_amd.recon import colorization, prepare_inputs, visulization
    g = load_golden("main_py")
    c = load_golden("pipeline257_color")
    segm = torch.from_numpy(g["segm"]).to(DEV)
    for tag, (m, sd) in {"cfg": ([0.5, 0.5, 0.5], [0.5, 0.5, 0.5]), "imagenet": ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])}.items():
        got_g, got_c = prepare_inputs(segm, m, sd)
        assert np.array_equal(got_g.cpu().numpy(), g["input_netG_" + tag]), tag   # bit for bit
        assert np.array_equal(got_c.cpu().numpy(), g["input_netC"])
    # the normal branch of colorization on the reference's vertices = the reference closure's render, bit for bit
    X = torch.from_numpy(c["X"].astype(np.int64)).to(DEV)
    Y = torch.from_numpy(c["Y"].astype(np.int64)).to(DEV)
    norm = torch.from_numpy(c["norm"]).to(DEV)
    rn = colorization(None, None, X, Y, torch.from_numpy(c["Z"]).to(DEV), torch.from_numpy(c["calib"]).to(DEV), norm)
    assert np.array_equal(rn.cpu().numpy(), c["norm_image"])
    vn, vt, vm = visulization(rn, torch.from_numpy(c["tex_image"]).to(DEV))
    assert np.array_equal(vn, g["vis_norm"]) and np.array_equal(vt, g["vis_tex"]) and np.array_equal(vm, g["vis_mask"])
    n2, t2, m2 = visulization(torch.from_numpy(g["vis129_in"]).to(DEV), None)
    assert t2 is None and np.array_equal(n2, g["vis129_norm"]) and np.array_equal(m2, g["vis129_mask"])


def test_bench_two_ranks_on_one_gpu():
    """bench.py's N > 1 path (rank-sharded frames, barriers, gather to rank 0, MAX-over-ranks
    timing) with two processes on this box's single GPU, launched the way the driver launched its
    N = 1 run -- plain ``python bench.py --gpus 2``, no torchrun: bench.py starts its own ranks.
    The test hook swaps RCCL for gloo; the rest of the code is what the 8-GPU run executes."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MONOPORT_BENCH_ONE_GPU_TEST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4",
           "--warmup", "2", "--depth", "1", "--batch", "2", "--passes", "2", "--full"]
    res = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["scaling"] == "weak"
    assert out["value"] > 0 and "cpu_baseline" not in out and 0 < out["roofline"]["frac"] < 1
    cfg = out["config"]
    assert cfg["self_launched"] is True and cfg["gather_checked"] is True and len(cfg["devices"]) == 2
    assert len(out["ms_per_step_per_rank"]) == 2 and out["passes"]["n"] == 2
    assert out["passes"]["value_min"] <= out["value"] <= out["passes"]["value_max"]
    assert 0 < out["scaling_vs_single_rank"]["efficiency"]
    # configs[3] at N = 2: 8 frames in flight = 2 slots x 2 frames per rank
    assert out["in_flight_8"]["value"] > 0 and "2 slot(s) x 2 frame(s)" in out["in_flight_8"]["config"]


def test_bench_collectives_on_rccl_one_rank_group():
    """The same collective calls on the REAL backend: `MONOPORT_BENCH_FORCE_GROUP=1` makes bench.py join a
    one-rank RCCL ("nccl") group and run the N > 1 code with it -- communicator creation with `device_id`,
    barrier, all_reduce on device tensors, all_gather_object, the gather of the renders on the slot's stream
    next to the encoder's hipGraph, the single-rank leg.  (Two ranks need two GPUs; this box has one.)"""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MONOPORT_BENCH_FORCE_GROUP="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
           "--passes", "2", "--full", "--no-extras"]
    res = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    cfg = out["config"]
    assert out["n_gpus"] == 1 and out["value"] > 0 and 0 < out["roofline"]["frac"] < 1
    assert "RCCL" in cfg["backend"] and cfg["gather_checked"] is True
    assert cfg["gather_ms_per_submission"]["median"] > 0
    assert 0.5 < out["scaling_vs_single_rank"]["efficiency"] < 1.5


def test_bench_dump_outputs_of_the_last_step(tmp_path):
    """bench.py --dump-outputs DIR: the last timed step's render, status row, vertices and volume sample as float32 /
    float64 .npy files within 64 MB -- and, the inputs being seeded, the same files from a second run of the same
    command (what lets two builds be compared output for output).  The runs are plain ones (no --full): the headline
    alone, none of the other legs."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
               "--passes", "1", "--dump-outputs", str(d)]
        res = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, res.stderr[-3000:]
        lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        out = json.loads(lines[0])
        assert out["steps"] == 4 and out["dumped_outputs"]["frame"] == 4 + 2 - 1
        assert out["value"] > 0 and out["ms_per_step"] > 0 and out["passes"]["n"] == 1
        assert not {"roofline", "breakdown", "plain_query_path", "final_level_rules", "two_slot_submissions",
                    "in_flight_8", "alt_precision", "mesh", "with_color", "levels6_f16w", "dropin",
                    "cpu_baseline"} & set(out)
        files = sorted(os.listdir(d))
        assert files == out["dumped_outputs"]["files"]
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        assert arrays["render"].shape == (257, 257, 3) and arrays["status"][0] == 1 and arrays["status"][1] == 17 ** 3
        n = arrays["vertices_x"].shape[0]
        assert n > 0 and arrays["vertices_y"].shape == arrays["vertices_z"].shape == (n,)
        assert arrays["vertices_normal"].shape == (n, 3)
        v = arrays["volume_sample"]
        assert v.shape == (1 << 22,) and 0 < float((v > 0.5).mean()) < 1
        dumps.append(arrays)
    for name, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][name]), name


def test_netg_query_uses_the_skip_table_by_default(monkeypatch):
    """MonoPortNet.bind makes and registers the skip table of a newly bound feature map
    (ops.SKIP_TABLE, default on): netG.query and the fused octree engine then blend table rows.  The
    field equals the plain path's up to f32 rounding; Seg3dLossless validates and fuses as before."""
    from monoport_amd import ops
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.recon import pifu_calib
    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", noise=0.05, seed=81))
    netG.to(DEV).eval()
    feats = [[torch.from_numpy(syn.body_feat(256, 128, 128, 4))[None].to(DEV)]]
    calib = pifu_calib(*syn.scene_camera(35), device=DEV)
    pts = torch.from_numpy(syn.rand_points(30000, 3, 1.0))[None].to(DEV)

    def query_func(points, feats, calib):
        return netG.query(feats, points.permute(0, 2, 1), calib)[0]

    res = [17, 33, 65, 129]
    box = dict(b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]), resolutions=res)
    got = {}
    for flag in (True, False):
        monkeypatch.setattr(ops, "SKIP_TABLE", flag)
        netG._hwc_cache.clear()  # a fresh bind (the cache key is the source tensors)
        out = netG.query(feats, pts, calib)[0]
        eng = Seg3dLossless(query_func=query_func, faster=True, **box).to(DEV)
        sdf = eng(feats=feats, calib=calib)
        assert eng.last_path == "fused"
        got[flag] = (out.clone(), sdf.clone(), eng.last_status.clone())
        assert netG.has_skip_table() == flag
    d = (got[True][0] - got[False][0]).abs().max().item()
    print("netG.query: |skip table - plain| = %.3g" % d)
    assert 0 < d <= 2e-6
    assert (got[True][1] - got[False][1]).abs().max().item() <= 2e-6
    # a voxel whose value sits within rounding of the threshold may land on either side
    assert int(((got[True][1] > 0.5) != (got[False][1] > 0.5)).sum()) <= 4


def test_reloaded_head_never_meets_a_stale_skip_table(monkeypatch):
    """A skip table holds products of the head's weights.  load_state_dict re-packs new weights into
    the SAME PackedMLP (same device buffer), so a table made before the reload would blend the old
    layer 0 / skip rows into the new hidden layers: mp_mlp_load forgets the head's tables and
    MonoPortNet.bind keys its cached table on the head's load generation.  After a reload the
    table path must agree with the plain path on the NEW weights -- through the module and at the
    ops / C-ABI level."""
    from monoport_amd import ops
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.recon import pifu_calib
    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", noise=0.05, seed=81))
    netG.to(DEV).eval()
    feats = [[torch.from_numpy(syn.body_feat(256, 128, 128, 4))[None].to(DEV)]]
    calib = pifu_calib(*syn.scene_camera(35), device=DEV)
    pts = torch.from_numpy(syn.rand_points(30000, 3, 1.0))[None].to(DEV)
    old = netG.query(feats, pts, calib)[0].clone()
    assert netG.has_skip_table()
    mlp_before = netG.surface_classifier.packed()
    _load_mlp(netG, syn.rand_mlp("G", 91, 2.0))  # other weights, same modules / same PackedMLP
    new_tab = netG.query(feats, pts, calib)[0].clone()
    assert netG.surface_classifier.packed() is mlp_before and netG.has_skip_table()
    monkeypatch.setattr(ops, "SKIP_TABLE", False)
    new_plain = netG.query(feats, pts, calib)[0].clone()
    assert not netG.has_skip_table()  # switching the flag off releases the cached table
    d_old = (new_tab - old).abs().max().item()
    d = (new_tab - new_plain).abs().max().item()
    print("reloaded head: |table - plain| = %.3g, |new - old| = %.3g" % (d, d_old))
    assert d_old > 1e-2 and d <= 2e-6
    # ops level: a table registered by hand is forgotten by load_layer (the C side drops it)
    layers_a, layers_b = syn.body_mlp("G", noise=0.05, seed=81), syn.rand_mlp("G", 91, 2.0)
    mlp = ops.PackedMLP.from_layers(DEV, layers_a, syn.LAST_OP["G"])
    fh = ops.pack_features(feats[0][0])
    handle = ops.skip_table(mlp, fh)
    with_table = ops.query(mlp, fh, pts, calib, syn.Z_SCALE).clone()
    for i, (w, b) in enumerate(layers_b):
        mlp.load_layer(i, torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV))
    after = ops.query(mlp, fh, pts, calib, syn.Z_SCALE).clone()  # plain kernels: no table left for fh
    ref = ops.query(ops.PackedMLP.from_layers(DEV, layers_b, syn.LAST_OP["G"]), fh, pts, calib, syn.Z_SCALE)
    handle.release()
    assert torch.equal(after, ref) and (after - with_table).abs().max().item() > 1e-2


def test_small_queries_do_not_build_a_skip_table():
    """MonoPortNet.bind makes the 16 GFLOP / 126 MB table only for the octree engine or once the map
    has served ops.SKIP_TABLE_MIN_POINTS points; a few small netG.query calls stay on the plain
    kernels (bit-identical to ops.query without a table)."""
    from monoport_amd import ops
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.recon import pifu_calib
    assert ops.SKIP_TABLE and ops.SKIP_TABLE_MIN_POINTS == 16384
    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", noise=0.05, seed=81))
    netG.to(DEV).eval()
    feats = [[torch.from_numpy(syn.body_feat(256, 128, 128, 4))[None].to(DEV)]]
    calib = pifu_calib(*syn.scene_camera(35), device=DEV)
    pts = torch.from_numpy(syn.rand_points(6000, 3, 1.0))[None].to(DEV)
    a = netG.query(feats, pts, calib)[0].clone()
    b = netG.query(feats, pts, calib)[0].clone()
    assert not netG.has_skip_table() and torch.equal(a, b)  # 12 k points served: plain path
    plain = ops.query(netG.surface_classifier.packed(), next(reversed(netG._hwc_cache.values()))[1], pts, calib, syn.Z_SCALE)
    assert torch.equal(a, plain)
    c = netG.query(feats, pts, calib)[0].clone()  # 18 k: the map has earned its table
    assert netG.has_skip_table()
    assert 0 < (c - a).abs().max().item() <= 2e-6
    # a new map starts over ... unless the octree engine binds it
    feats2 = [[torch.from_numpy(syn.body_feat(256, 128, 128, 5))[None].to(DEV)]]
    netG.query(feats2, pts, calib)
    assert not netG.has_skip_table()
    eng = Seg3dLossless(query_func=lambda points, feats, calib: netG.query(feats, points.permute(0, 2, 1), calib)[0],
                        b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]),
                        resolutions=[9, 17, 33], faster=True).to(DEV)
    eng(feats=feats2, calib=calib)
    assert eng.last_path == "fused" and netG.has_skip_table()


def test_trusted_query_func_is_validated_again_periodically():
    """After VALIDATE_CALLS agreeing frames the engine trusts query_func and only probes it -- but
    every REVALIDATE_EVERY-th call is validated for real again, so a wrapper whose arithmetic
    changes later (here: `1 - pred` from some frame on) is caught and honoured through the generic
    engine instead of being bypassed for good."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.recon import pifu_calib
    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", noise=0.05, seed=81))
    netG.to(DEV).eval()
    feats = [[torch.from_numpy(syn.body_feat(256, 128, 128, 4))[None].to(DEV)]]
    calib = pifu_calib(*syn.scene_camera(35), device=DEV)
    state = {"flip": False, "calls": []}

    def query_func(points, feats, calib):
        state["calls"].append(points.shape[1])
        pred = netG.query(feats, points.permute(0, 2, 1), calib)[0]
        return 1 - pred if state["flip"] else pred

    eng = Seg3dLossless(query_func=query_func, b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]),
                        resolutions=[9, 17, 33], faster=True, validate="first").to(DEV)
    eng.REVALIDATE_EVERY = 4
    for _ in range(3 + 8):
        eng(feats=feats, calib=calib)
        assert eng.last_path == "fused"
    # 3 validated, then (3 probes, 1 validated) twice
    assert state["calls"] == [729] * 3 + [1, 1, 1, 729] * 2
    inside = eng(feats=feats, calib=calib)
    state["flip"] = True
    paths = []
    import warnings as _w
    with _w.catch_warnings():
        _w.simplefilter("ignore")
        for _ in range(4):
            out = eng(feats=feats, calib=calib)
            paths.append(eng.last_path)
    assert "generic" in paths and paths[-1] == "generic"  # caught within REVALIDATE_EVERY frames, stays caught
    assert (((out > 0.5) != (inside > 0.5)).float().mean().item()) > 0.5  # the flipped field is what comes back
    # the class default (validate="always") honours the change on the very frame it happens
    state["flip"] = False
    dflt = Seg3dLossless(query_func=query_func, b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]),
                         resolutions=[9, 17, 33], faster=True).to(DEV)
    for _ in range(5):
        dflt(feats=feats, calib=calib)
        assert dflt.last_path == "fused"
    state["flip"] = True
    with _w.catch_warnings():
        _w.simplefilter("ignore")
        out = dflt(feats=feats, calib=calib)
    assert dflt.last_path == "generic"
    assert (((out > 0.5) != (inside > 0.5)).float().mean().item()) > 0.5


def test_coalesced_stages_give_the_per_frame_results():
    """stage_pipeline.Coalesced + Seg3dLossless.forward_many + forward_vertices_many: a recon stage that
    serves several queued frames with one mp_recon_batch returns, per frame, exactly what the per-frame
    stage returns (volumes and vertices bit for bit), in FIFO order; an untrusted engine serves the
    frames one by one."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    from monoport_amd.modeling import PIFuNetG
    from monoport_amd.recon import forward_vertices, forward_vertices_many, pifu_calib
    from monoport_amd.stage_pipeline import Coalesced, StagePipeline
    netG = PIFuNetG()
    _load_mlp(netG, syn.body_mlp("G", noise=0.05, seed=81))
    netG.to(DEV).eval()

    def query_func(points, feats, calib):
        return netG.query(feats, points.permute(0, 2, 1), calib)[0]

    res = [9, 17, 33, 65]
    eng = Seg3dLossless(query_func=query_func, b_min=np.array([[-1., -1., -1.]]), b_max=np.array([[1., 1., 1.]]),
                        resolutions=res, faster=True, validate="first").to(DEV)  # batching needs a trusted closure
    frames = [dict(feats=[[torch.from_numpy(syn.body_feat(256, 128, 128, 4 + i))[None].to(DEV)]],
                   calib=pifu_calib(*syn.scene_camera(10 * i), device=DEV)) for i in range(6)]
    many0 = eng.forward_many(frames[:3])  # not validated yet: frame by frame through forward()
    assert eng._agreed == 3 and eng.last_path == "fused"
    singles = [eng(**f) for f in frames]
    verts = [forward_vertices(s) for s in singles]
    batch = eng.forward_many(frames)  # trusted now: one mp_recon_batch
    assert all(torch.equal(a, b) for a, b in zip(batch, singles)) and all(torch.equal(a, b) for a, b in zip(many0, singles[:3]))
    for v, w in zip(forward_vertices_many(batch), verts):
        assert all(torch.equal(a, b) for a, b in zip(v, w))
    # through the pipeline: the recon stage is held back until five frames wait in front of it
    import threading
    gate, sizes = threading.Event(), []

    def hold(d):
        if d["i"] == 0:
            gate.wait(10)
        return d

    def many(ds):
        sizes.append(len(ds))
        return [{**d, "sdf": s} for d, s in zip(ds, eng.forward_many([frames[d["i"]] for d in ds]))]

    def source():
        for i in range(6):
            yield {"i": i}
        gate.set()

    stages = [Coalesced(hold, lambda ds: [hold(d) for d in ds], 8),
              Coalesced(lambda d: {**d, "sdf": eng(**frames[d["i"]])}, many, max_batch=8)]
    with torch.no_grad():
        outs = list(StagePipeline(source(), stages, device=DEV, max_in_flight=8))
    assert [d["i"] for d in outs] == list(range(6)) and max(sizes) > 1
    assert all(torch.equal(d["sdf"], singles[d["i"]]) for d in outs)


def test_soak_of_the_per_frame_pipeline_is_flat_and_surfaces_errors():
    """The reference's steady-state mode (RTL/main.py:487: an endless loop at one frame per stage call) for ~10 s
    on 64 rotating images / cameras with empty scenes in the mix (bench_dropin.soak, the `dropin.soak` leg of
    bench.py): every frame comes back, empty scenes as None (RTL/recon.py:32-33), and after the first window
    nothing the process holds grows -- torch's reserved bytes, the C side's arenas / weights / registered tables
    (mp_memory_stats), the encoder's recorded plans.  Then the same pipeline with a failure injected in the recon
    stage: the error reaches the consumer (RTL/dataloader.py:1042-1047) and every stage thread exits."""
    import bench_dropin
    res = bench_dropin.soak(DEV, 10.0, [17, 33, 65, 129, 257], window_s=2.5, empty_every=23)
    lat = res["latency_ms"]
    print("soak: %d frames in %.1f s = %.1f recon/s, %d None; latency p50 %.1f p99 %.1f max %.1f ms; windows %s"
          % (res["frames"], res["seconds"], res["value"], res["none_frames"], lat["p50"], lat["p99"], lat["max"],
             [(round(w["value"], 1), w["torch_reserved"] >> 20, w["mp_arena_bytes"] >> 20, w["mp_arenas"],
               w["mp_skip_tables"], w["encoder_plans"]) for w in res["windows"]]))
    assert res["error"] is None and res["stage_threads_alive_after"] == 0
    assert res["frames"] > 300 and res["none_frames"] == res["frames"] // 23
    assert len(res["windows"]) >= 3 and res["flat_after_warmup"], res["windows"]
    steady = res["latency_ms_after_first_window"]  # the first window records the plan and grows pools / arenas
    print("after the first window: p50 %.1f p99 %.1f max %.1f ms" % (steady["p50"], steady["p99"], steady["max"]))
    assert steady["p99"] < 2 * steady["p50"] and steady["max"] < 4 * steady["p50"]  # no stall once warm
    sweep = res["latency_by_frames_in_flight"]
    print("latency by frames in flight:", {k: (round(v["value"], 1), round(v["latency_ms"]["p50"], 2), round(v["latency_ms"]["p99"], 2))
                                          for k, v in sweep.items()})
    assert sweep["1"]["latency_ms"]["p50"] < sweep["4"]["latency_ms"]["p50"] < lat["p50"]  # Little's law
    bad = bench_dropin.soak(DEV, 3.0, [17, 33, 65, 129, 257], window_s=1.0, raise_at=40)
    assert bad["error"] is not None and "stage 5 failed" in bad["error"] and "injected failure at frame 40" in bad["error"]
    assert bad["frames"] == 40 and bad["stage_threads_alive_after"] == 0
