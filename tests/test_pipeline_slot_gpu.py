"""The configuration the headline of bench.py measures, held to float64 frame by frame: FramePipeline slots of 20 and
32 frames (bench.pick_batch), the encoder as a captured hipGraph writing the channels-last map itself
(FrameSlot.hwc_direct), skip tables over the whole slot, three slots submitted back to back.

At these batches the 3x3 launcher picks other kernels than at batch 1-4 (the Winograd threshold of 128 workgroups,
the 128-channel Winograd kernel once tiles * n * cout / 128 >= 2048, the direct kernel's tile / split-K choice, the
GroupNorm statistics slices), so the whole encoder is compared with a float64 copy of itself on every 3x3 route, and
the slot's results are split into two checks: its features against float64, and everything downstream of them
against the single-frame calls on those same features, bit for bit (recon_batch == recon, paint_batch == paint and
query_counted_batch == query_counted are contracts of their own).  The bench's other legs are built and checked
the same way: f16x3 encoder and head in slots of 16 / 10 (`alt_precision`), 17..513 with the f16w head in slots of
16 (`levels6_f16w`), the upstream / interpolate last levels (`final_level_rules`) and two slots of 4 in flight
(`in_flight_8`).  Needs an MI355X."""
import time

import numpy as np
import pytest

from conftest import check_full_coverage, load_golden
from monoport_amd import synthetic as syn

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

ENCODER_BAR = 1e-4  # the encoders against the reference (tests/test_encoder_dataflow_gpu.py)
PIN_BAR = 2e-5      # the float64 copy against the reference's own f32 output
DIRECT, K64, K128 = 0x400, 0x800, 0x1000
ROUTES = {"auto": 0, "direct": DIRECT, "wino64": K64, "wino128": K128}
N_DISTINCT = 32  # distinct synthetic images; frame f of a stream shows image f % N_DISTINCT
# encoder entry points a float64 module must never reach: a fall-through to HIP would compare HIP with itself
HIP_ENTRY_POINTS = ("conv3x3_fused", "conv1x1_fused", "convk", "gn_apply", "avgpool2_gn", "upsample_add_gn",
                    "group_norm", "upsample_bicubic2x", "concat3_add", "conv3x3_gn", "conv1x1", "scale_shift_add",
                    "gn_stats", "gn_finalize", "pack_features")

_IMAGES = {}


def _image(seed):
    if seed not in _IMAGES:
        _IMAGES[seed] = torch.from_numpy(syn.synthetic_image(seed)).to(DEV)
    return _IMAGES[seed]


def _calib(frame):
    from monoport_amd.recon import pifu_calib
    return pifu_calib(*syn.scene_camera(3 * frame), device=DEV)  # bench.Job's cameras


def _float64_copy(module, fresh):
    """``fresh`` (a new module of the same architecture) with ``module``'s weights, in float64 on the GPU: every
    HIP path of modeling/backbones.py gates on float32, so this runs torch's own float64 operators."""
    fresh.load_state_dict(module.state_dict())
    return fresh.to(DEV).double().eval()


class Float64Encoders:
    """netG's HGFilter and netC's ResnetFilter in float64, one image at a time, memoised by image seed."""

    def __init__(self, netg, netc):
        from monoport_amd.modeling import PIFuNetC, PIFuNetG
        self.g = _float64_copy(netg.image_filter, PIFuNetG().image_filter)
        self.c = _float64_copy(netc.image_filter, PIFuNetC().image_filter)
        self._g, self._c = {}, {}
        self.seconds = {"g": [], "c": []}

    def _run(self, module, x):
        with pytest.MonkeyPatch.context() as mp, torch.no_grad():
            from monoport_amd import ops

            def refuse(*args, **kwargs):
                raise AssertionError("the float64 reference reached a HIP entry point")

            for name in HIP_ENTRY_POINTS:
                mp.setattr(ops, name, refuse)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = module(x.double()[None])
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        assert all(o[0].dtype == torch.float64 for o in out)
        return out, dt

    def netg(self, seed):
        """The four stacks' outputs of image ``seed``: [4,256,128,128] float64."""
        if seed not in self._g:
            out, dt = self._run(self.g, _image(seed))
            self._g[seed] = torch.stack([o[0][0] for o in out])
            self.seconds["g"].append(dt)
        return self._g[seed]

    def netc(self, seed):
        """ResnetFilter's output of image ``seed``: [256,128,128] float64."""
        if seed not in self._c:
            out, dt = self._run(self.c, _image(seed))
            self._c[seed] = out[0][0][0]
            self.seconds["c"].append(dt)
        return self._c[seed]


@pytest.fixture(scope="module")
def nets():
    import bench
    dev = torch.device(DEV)
    netg = bench.build_netg(dev)[0]
    netc = bench.build_netc(dev)
    return netg, netc, Float64Encoders(netg, netc)


def test_float64_encoders_reproduce_the_reference(nets):
    """The yardstick first: on the `encoders` fixture's inputs (netG seed 71, netC seed 72, synthetic_image(73)) the
    float64 copies reproduce the reference's G0..G3 and C0 (its CPU f32 output) within 2e-5, sampled and through the
    8 x 8 block / pixel means of every element."""
    netg, netc, ref = nets
    gold = load_golden("encoders")
    g = ref.netg(73).cpu().numpy()
    errs = [float(np.abs(g[i][::8, ::8, ::8] - gold["G%d" % i]).max()) for i in range(4)]
    eb, ep = check_full_coverage(gold, "G3", g[3], tol=PIN_BAR)
    c0 = np.concatenate([g[3], ref.netc(73).cpu().numpy()])
    err_c = float(np.abs(c0[::8, ::8, ::8] - gold["C0"]).max())
    ebc, epc = check_full_coverage(gold, "C0", c0, tol=PIN_BAR)
    print("float64 encoders vs the reference's f32: G0..G3 %s (G3 block means %.3g, pixel means %.3g), C0 %.3g "
          "(block %.3g, pixel %.3g); one image in float64: HGFilter %.2f s, ResnetFilter %.2f s"
          % (["%.3g" % e for e in errs], eb, ep, err_c, ebc, epc, ref.seconds["g"][0], ref.seconds["c"][0]))
    assert max(errs) <= PIN_BAR and err_c <= PIN_BAR


def _checked(n):
    return sorted({0, n // 2, n - 1})


@pytest.mark.parametrize("n,route", [(n, r) for n in (13, 20, 32) for r in ("auto", "direct", "wino64")]
                         + [(32, "wino128")])
def test_whole_encoder_at_slot_batches_vs_float64(nets, n, route):
    """HGFilter at the slot batches on each 3x3 route (the heuristic, forced direct kernels, forced 64- / 128-channel
    Winograd kernels): every stack of images 0, n/2 and n-1 against float64 (1e-4), every image against the same
    image at batch 1 on the same route (1e-4), and a second pass bit for bit."""
    from monoport_amd import _lib
    netg, _, ref = nets
    enc = netg.image_filter
    lib = _lib.load()
    imgs = torch.stack([_image(s % N_DISTINCT) for s in range(n)])
    lib.mp_conv3x3_tune(ROUTES[route])
    try:
        with torch.no_grad():
            out = torch.stack([o[0] for o in enc(imgs, graphed=False)])  # [4,n,256,128,128]
            again = enc(imgs, graphed=False)
            same = all(torch.equal(out[k], again[k][0]) for k in range(4))
            del again
            d_b = torch.zeros((), device=DEV)
            for i in range(n):
                one = torch.stack([o[0][0] for o in enc(imgs[i:i + 1], graphed=False)])
                d_b = torch.maximum(d_b, (out[:, i] - one).abs().max())
    finally:
        lib.mp_conv3x3_tune(0)
    errs = {i: [(out[k, i].double() - ref.netg(i % N_DISTINCT)[k]).abs().max().item() for k in range(4)]
            for i in _checked(n)}
    err = max(max(e) for e in errs.values())
    print("HGFilter batch %d, %s 3x3 route: vs float64 max %.3g (per image, stacks 0..3: %s); batch %d vs batch 1 "
          "%.3g" % (n, route, err, {i: ["%.2g" % v for v in e] for i, e in errs.items()}, n, d_b.item()))
    assert same, "second pass differs"
    assert err <= ENCODER_BAR and d_b.item() <= ENCODER_BAR


def test_encoder_hwc_output_at_batch_32(nets):
    """What a 32-frame slot asks for -- last_only with the channels-last map written by the producing kernel -- equals
    mp_feat_pack_hwc of the NCHW output of the same pass bit for bit (test_encoder_hwc_output_equals_packed_nchw at
    batch 2), and the pass without hwc_out."""
    from monoport_amd import ops
    netg, _, _ = nets
    enc = netg.image_filter
    imgs = torch.stack([_image(s % N_DISTINCT) for s in range(32)])
    hwc = torch.full((32, 128, 128, 256), float("nan"), device=DEV)
    with torch.no_grad():
        got = enc(imgs, last_only=True, hwc_out=hwc, keep_nchw=True, graphed=False)[-1][0]
        plain = enc(imgs, last_only=True, graphed=False)[-1][0]
        only = enc(imgs, last_only=True, hwc_out=torch.empty_like(hwc), graphed=False)
    assert only[-1][0] is None and torch.equal(got, plain)
    for b in (0, 15, 31):
        assert torch.equal(hwc[b], ops.pack_features(got[b:b + 1])), b


def test_encoder_f16x3_at_batch_32_vs_float64(nets):
    """f16x3 (f32 emulated on f16 MFMA) at 32 frames: every stack within the 1e-4 the f16x3 encoder is held to
    against the reference (test_hgfilter_dataflow_vs_reference_and_round2_path)."""
    import bench
    netg, _, ref = nets
    imgs = torch.stack([_image(s % N_DISTINCT) for s in range(32)])
    bench.set_precision_everywhere(netg.surface_classifier, "f16x3")
    try:
        with torch.no_grad():
            out = torch.stack([o[0] for o in netg.image_filter(imgs, graphed=False)])
            again = netg.image_filter(imgs, graphed=False)
            same = all(torch.equal(out[k], again[k][0]) for k in range(4))
    finally:
        bench.set_precision_everywhere(netg.surface_classifier, "f32")
    err = max((out[k, i].double() - ref.netg(i)[k]).abs().max().item() for i in _checked(32) for k in range(4))
    print("HGFilter f16x3 batch 32: vs float64 max %.3g" % err)
    assert same and err <= ENCODER_BAR


def test_netc_filter_with_prior_at_batch_20_vs_float64(nets):
    """netC.filter(images, feat_prior = netG's last stack) at 20 frames: the prior and ResnetFilter's output against
    float64 (1e-4)."""
    netg, netc, ref = nets
    imgs = torch.stack([_image(s % N_DISTINCT) for s in range(20)])
    with torch.no_grad():
        prior = netg.image_filter(imgs, graphed=False)[-1][0]
        fc = netc.filter(imgs, feat_prior=prior)[0][0]
    assert fc.shape == (20, 512, 128, 128)
    err = max((fc[i].double() - torch.cat([ref.netg(i)[3], ref.netc(i)])).abs().max().item() for i in _checked(20))
    print("netC.filter with feat_prior, batch 20: vs float64 max %.3g" % err)
    assert err <= ENCODER_BAR


def _run_bench_slots(batch, n_frames, warm, with_color, precision="f32", resolutions=None, final_level="dilate3",
                     depth=3):
    """bench.make_pipeline's pipeline (``depth`` slots, hipGraph encoder; bench.RESOLUTIONS, f32 and the dilate3 last
    level unless told otherwise); ``warm`` frames, then ``n_frames`` frames submitted back to back as
    bench.timed_passes does, with a device-side snapshot of every submission's results on the slot's stream (no host
    sync).  Returns (snapshots, slot-0 facts).  bench.build_netg(dev, "f16x3") switches the encoder's 3x3
    convolutions to f16x3 process-wide: the switch is set back to f32 before this returns."""
    import bench
    from monoport_amd.modeling import backbones
    try:
        pipe = bench.make_pipeline(torch.device(DEV), depth, True, resolutions or bench.RESOLUTIONS, with_color,
                                   precision, batch, final_level)
        try:
            s = pipe.slots[0]
            assert all(sl.hwc_direct and sl.graph is not None for sl in pipe.slots)
            assert s.net.surface_classifier.precision == precision and s.final_level == final_level
            facts = {"mlp": s.net.surface_classifier.packed(), "tables": s.tables is not None,
                     "mlp_c": s.netC.surface_classifier.packed() if with_color else None,
                     "mat_color": s.mat_color if with_color else None,
                     "res": list(s.res), "final_level": s.final_level}
            snaps = []
            total = warm + n_frames
            for s0 in range(0, total, batch):
                s1 = min(s0 + batch, total)
                frames = list(range(s0, s1))
                slot = pipe.submit([_image(f % N_DISTINCT)[None] for f in frames], [_calib(f) for f in frames])
                if s0 < warm:
                    continue
                n = s1 - s0
                assert slot.n_active == n
                with torch.cuda.stream(slot.stream):
                    snap = {"frames": frames, "feat": slot.feat_hwc_all[:n].clone(),
                            "status": slot.status[:n].clone(),
                            "render": [slot.renders[b].clone() for b in range(n)],
                            "volume": [slot.volumes[b].clone() for b in range(n)]}
                    if with_color:
                        snap["feat_c"] = [slot.feats_hwc_c[b].clone() for b in range(n)]
                        snap["tex"] = [slot.renders_tex[b].clone() for b in range(n)]
                snaps.append(snap)
            pipe.synchronize()
        finally:
            pipe.close()
    finally:
        backbones.set_encoder_conv_precision("f32")
    torch.cuda.synchronize()
    return snaps, facts


def _single_frame_geometry(facts, feat, calib):
    """The single-frame calls on one frame's features, with the slot's head (its precision), grids and last-level
    rule: skip table (when the slot makes them), octree, visible vertices, normal render."""
    from monoport_amd import ops
    import bench
    table = ops.skip_table(facts["mlp"], feat) if facts["tables"] else None
    try:
        vol, st = ops.recon(facts["mlp"], feat, calib, syn.Z_SCALE, bench.B_MIN, bench.B_MAX, facts["res"],
                            final_level=facts["final_level"])
        raw = ops.forward_vertices_raw(vol, "front")
        x, y, _, nrm, count = raw
        render = ops.paint(x, y, nrm, 0, count, facts["res"][-1], 0.5, 0.5, 0.0, 1.0)
        torch.cuda.synchronize()
    finally:
        if table is not None:
            table.release()
    return st, vol, raw, render


def _check_slot_frames(snaps, facts, ref, f64_positions):
    """Per frame: hook channels exact, features vs float64 where asked, downstream of the features bit for bit.
    Returns the largest feature error against float64."""
    from monoport_amd import ops
    planes = torch.from_numpy(syn.body_feature_planes(128, 128)).to(DEV).permute(1, 2, 0)
    worst = 0.0
    n_checked = 0
    for snap in snaps:
        n = len(snap["frames"])
        for b, f in enumerate(snap["frames"]):
            feat = snap["feat"][b]
            assert torch.equal(feat[..., 0:2], planes), "frame %d: hook channels" % f
            if b in f64_positions(n):
                want = ref.netg(f % N_DISTINCT)[3].permute(1, 2, 0)
                err = (feat[..., 2:].double() - want[..., 2:]).abs().max().item()
                worst = max(worst, err)
                n_checked += 1
                assert err <= ENCODER_BAR, "frame %d (slot of %d, entry %d): features vs float64 %.3g" % (f, n, b, err)
            calib = _calib(f)
            st, vol, raw, render = _single_frame_geometry(facts, feat, calib)
            assert torch.equal(st, snap["status"][b]), "frame %d: octree status" % f
            assert int(st[0]) == 1
            assert torch.equal(vol, snap["volume"][b]), "frame %d: volume" % f
            assert torch.equal(render, snap["render"][b]), "frame %d: render" % f
            if facts["mlp_c"] is not None:
                feat_c = snap["feat_c"][b]
                assert torch.equal(feat_c[..., :256], feat), "frame %d: netC's prior is not netG's map" % f
                x, y, z, _, count = raw
                r = facts["res"][-1]
                pts = ops.vertex_points(x, y, z, count, r, facts["mat_color"])
                pred = ops.query_counted(facts["mlp_c"], feat_c, pts, count, calib, syn.Z_SCALE)
                tex = ops.paint(x, y, pred, 1, count, r, 0.5, 0.5, -np.inf, np.inf)
                assert torch.equal(tex, snap["tex"][b]), "frame %d: texture render" % f
    assert n_checked >= 2 * len(snaps)
    return worst


@pytest.mark.parametrize("batch,n_frames,warm", [(20, 45, 20), (32, 64, 0)])
def test_bench_slot_frame_by_frame(nets, batch, n_frames, warm):
    """The bench's own slots: 45 frames at batch 20 (20 + 20 + 5, the short slot on a slot whose other 15 entries hold
    the images of an earlier submission) and 64 at batch 32.  Every frame: channels 0/1 = body_feature_planes exactly;
    first, middle and last frame of every slot: channels 2..255 against the float64 encoder of the frame's image (1e-4);
    status, volume and render = the single-frame calls on the slot's own features, bit for bit."""
    _, _, ref = nets
    t0 = time.perf_counter()
    snaps, facts = _run_bench_slots(batch, n_frames, warm, False)
    assert [len(s["frames"]) for s in snaps] == ([20, 20, 5] if batch == 20 else [32, 32])
    worst = _check_slot_frames(snaps, facts, ref, lambda n: {0, n // 2, n - 1})
    print("bench slot of %d, %d frames: features vs float64 max %.3g; status / volume / render of every frame equal the "
          "single-frame calls (%.1f s)" % (batch, n_frames, worst, time.perf_counter() - t0))


def test_bench_colour_slot_frame_by_frame(nets):
    """BASELINE configs[2] in the bench's slots of 20 (45 frames, a short last slot): the geometry checks above, plus
    netC's channels-last map of every frame = [netG's map | ResnetFilter's output] with the second half against
    float64 on two frames, and the texture render = vertex_points -> query_counted (netC head) -> paint on the slot's
    own map, bit for bit."""
    _, _, ref = nets
    t0 = time.perf_counter()
    snaps, facts = _run_bench_slots(20, 45, 20, True)
    worst = _check_slot_frames(snaps, facts, ref, lambda n: {0, n - 1})
    worst_c = 0.0
    for snap, b in ((snaps[0], 0), (snaps[-1], len(snaps[-1]["frames"]) - 1)):
        f = snap["frames"][b]
        want = ref.netc(f % N_DISTINCT).permute(1, 2, 0)
        worst_c = max(worst_c, (snap["feat_c"][b][..., 256:].double() - want).abs().max().item())
    print("bench colour slot of 20, 45 frames: netG features vs float64 max %.3g, netC features %.3g; geometry and "
          "texture renders equal the single-frame calls (%.1f s)" % (worst, worst_c, time.perf_counter() - t0))
    assert worst_c <= ENCODER_BAR


def _oracle_decisions(oracle, facts, feat, calib):
    """oracle.seg3d_lossless (the CPU restatement of the octree) with the slot's grids and last-level rule, driven
    by the slot's HIP query kernel on one frame's features (through the frame's skip table when the slot makes
    them): (volume, points per level).  Both sides get their occupancies from the same kernel, so they take the
    same decisions and give the same volume bits."""
    import bench
    from monoport_amd import ops
    table = ops.skip_table(facts["mlp"], feat) if facts["tables"] else None
    try:
        def gpu_query(pts):
            return ops.query(facts["mlp"], feat, torch.from_numpy(np.ascontiguousarray(pts))[None].to(DEV), calib,
                             syn.Z_SCALE)[0, 0].cpu().numpy()

        stats = []
        vol = oracle.seg3d_lossless(gpu_query, bench.B_MIN, bench.B_MAX, facts["res"], stats=stats,
                                    final_level=facts["final_level"])
    finally:
        if table is not None:
            table.release()
    return vol, stats


@pytest.mark.parametrize("steps,n_frames", [(32, 40), (20, 25)])
def test_bench_f16x3_slot_frame_by_frame(nets, steps, n_frames):
    """The bench's `alt_precision` leg as bench.py builds it: bench.make_pipeline(..., "f16x3",
    pick_batch(steps, 16)) -- slots of 16 frames at the default 32 steps and of 10 at --steps 20, here with a short
    last slot (16 + 16 + 8, 10 + 10 + 5).  The encoder's 3x3 convolutions and the query run f16x3; the f16x3 head
    reads skip tables.  Frames 0, n/2 and n-1 of every slot: features against float64 (1e-4); the first slot's
    features differ from the f32 encoder's at the same batch on the same images (the f16x3 kernels ran, not a
    stale f32 graph or pack); every frame: status, volume and render = the single-frame calls with the f16x3 head,
    bit for bit."""
    import bench
    from monoport_amd.modeling import backbones
    netg, _, ref = nets
    batch = bench.pick_batch(steps, 16)
    assert batch == {32: 16, 20: 10}[steps]
    t0 = time.perf_counter()
    snaps, facts = _run_bench_slots(batch, n_frames, 0, False, precision="f16x3")
    assert backbones.ENCODER_CONV_PRECISION == "f32"
    assert [len(s["frames"]) for s in snaps] == [batch, batch, n_frames - 2 * batch]
    assert facts["tables"] and facts["mlp"].precision == "f16x3"
    worst = _check_slot_frames(snaps, facts, ref, lambda n: {0, n // 2, n - 1})
    first = snaps[0]
    imgs = torch.stack([_image(f % N_DISTINCT) for f in first["frames"]])
    with torch.no_grad():
        f32 = netg.image_filter(imgs, last_only=True, graphed=False)[-1][0].permute(0, 2, 3, 1)
    moved = [(first["feat"][b, ..., 2:] - f32[b, ..., 2:]).abs().max().item() for b in _checked(batch)]
    del f32
    print("bench f16x3 slot of %d, %d frames: features vs float64 max %.3g, vs the f32 encoder at batch %d %s; "
          "status / volume / render of %d frames equal the single-frame calls (%.1f s)"
          % (batch, n_frames, worst, batch, ["%.3g" % d for d in moved], n_frames, time.perf_counter() - t0))
    assert all(d > 0 for d in moved), "f16x3 slot features equal the f32 encoder's"


def test_bench_levels6_f16w_slot_frame_by_frame(nets):
    """The bench's `levels6_f16w` leg (BASELINE configs[4]): bench.RESOLUTIONS + [513], f16w head, slots of
    pick_batch(32, 16) = 16 frames; 20 frames (16 + a short 4).  Features against float64 (1e-4); every frame's
    status, 513^3 volume and 513^2 render = the single-frame calls with the f16w head, bit for bit; frame 0's
    volume against the f32 head's volume on the same features and camera: IoU >= 0.9999 (the bench's own
    `iou_vs_f32_volume`, at the bar of test_config5_513_fp16_weights)."""
    import bench
    from monoport_amd import ops
    _, _, ref = nets
    res6 = bench.RESOLUTIONS + [513]
    batch = bench.pick_batch(32, 16)
    assert batch == 16
    t0 = time.perf_counter()
    snaps, facts = _run_bench_slots(batch, 20, 0, False, precision="f16w", resolutions=res6)
    assert [len(s["frames"]) for s in snaps] == [16, 4]
    assert facts["res"] == res6 and not facts["tables"] and facts["mlp"].precision == "f16w"
    worst = _check_slot_frames(snaps, facts, ref, lambda n: {0, n // 2, n - 1})
    mlp32 = ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", noise=0.05, seed=1), syn.LAST_OP["G"])
    vol32, st32 = ops.recon(mlp32, snaps[0]["feat"][0], _calib(0), syn.Z_SCALE, bench.B_MIN, bench.B_MAX, res6)
    occ32, occ16 = vol32 > 0.5, snaps[0]["volume"][0] > 0.5
    iou = (occ32 & occ16).sum().item() / max((occ32 | occ16).sum().item(), 1)
    del snaps, vol32, occ32, occ16
    torch.cuda.empty_cache()
    print("bench levels6_f16w slot of 16, 20 frames at 17..513: features vs float64 max %.3g; status / volume / "
          "render of 20 frames equal the single-frame calls; frame 0 IoU vs the f32 volume %.6f (%.1f s)"
          % (worst, iou, time.perf_counter() - t0))
    assert int(st32[0]) == 1 and iou >= 0.9999


@pytest.mark.parametrize("rule", ["upstream", "interpolate"])
def test_bench_final_level_slot_frame_by_frame(nets, oracle, rule):
    """The bench's `final_level_rules` leg: bench.make_pipeline(..., final_level=rule) in slots of 20, 45 frames
    after 20 warm-up frames (20 + 20 + 5: the short slot on a slot that held an earlier submission).  Features of
    frames 0, n/2, n-1 against float64; every frame's status, volume and render = the single-frame
    ops.recon(..., final_level=rule) calls, bit for bit; the last frame (of the short slot) = the CPU restatement
    oracle.seg3d_lossless(final_level=rule) driven by the same HIP query on the slot's own features."""
    _, _, ref = nets
    t0 = time.perf_counter()
    snaps, facts = _run_bench_slots(20, 45, 20, False, final_level=rule)
    assert [len(s["frames"]) for s in snaps] == [20, 20, 5]
    assert facts["final_level"] == rule
    worst = _check_slot_frames(snaps, facts, ref, lambda n: {0, n // 2, n - 1})
    last = torch.cat([s["status"][:, -1] for s in snaps])
    if rule == "interpolate":
        assert (last == 0).all()  # nothing is evaluated at 257^3
    else:
        assert (last > 0).all()
    t1 = time.perf_counter()
    snap = snaps[-1]
    b, f = len(snap["frames"]) - 1, snap["frames"][-1]
    want, stats = _oracle_decisions(oracle, facts, snap["feat"][b], _calib(f))
    t2 = time.perf_counter()
    assert snap["status"][b].tolist() == [1] + stats, "frame %d: points per level vs the CPU restatement" % f
    assert np.array_equal(snap["volume"][b].cpu().numpy(), want), "frame %d: volume vs the CPU restatement" % f
    print("bench slot of 20, final_level=%s, 45 frames: features vs float64 max %.3g; status / volume / render of "
          "45 frames equal the single-frame calls; frame %d = oracle.seg3d_lossless (points per level %s, %.1f s); "
          "%.1f s in all" % (rule, worst, f, stats, t2 - t1, time.perf_counter() - t0))


def test_bench_in_flight_8_slots_frame_by_frame(nets):
    """The bench's `in_flight_8` leg (BASELINE configs[3]): depth, batch = in_flight_layout(8, 1) = 2 slots of 4
    frames alternating on two streams; 16 frames back to back at bench.RESOLUTIONS.  Every frame's features against
    float64 (1e-4), and its status, volume and render = the single-frame calls, bit for bit."""
    import bench
    _, _, ref = nets
    depth, batch = bench.in_flight_layout(8, 1)
    assert (depth, batch) == (2, 4)
    t0 = time.perf_counter()
    snaps, facts = _run_bench_slots(batch, 16, 0, False, depth=depth)
    assert [len(s["frames"]) for s in snaps] == [4, 4, 4, 4]
    worst = _check_slot_frames(snaps, facts, ref, lambda n: set(range(n)))
    print("bench in_flight_8 (2 slots of 4), 16 frames: features of every frame vs float64 max %.3g; status / "
          "volume / render of 16 frames equal the single-frame calls (%.1f s)" % (worst, time.perf_counter() - t0))
