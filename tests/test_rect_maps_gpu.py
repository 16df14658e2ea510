"""Every kernel that samples a feature map, on maps with H != W (tests/rect_cases.py): ops.index, the plain f32
query kernels (64- and 32-point tiles, Cout = 1 and 3, C = 256 and 512, orthogonal and perspective), the skip table
and the query through it, the table registry, the three f16 kernels plain and through the table, the batched and
counted forms, the multi-view kernel, the fused reconstructions (lossless, batched, perspective, multi-view,
fixed-budget) and the Python layer above them.  Held to the fixture the reference produced (tests/golden/
rect_maps.npz), to the CPU oracle and to float64 at the bars the same kernels carry on square maps; one test per
kernel family also shows that the oracle on the exchanged map is far away, so an exchanged (h, w) cannot pass.
tests/test_rect_maps_cpu.py pins the yardsticks.  Needs an MI355X."""
import numpy as np
import pytest

import rect_cases as rc
from conftest import load_golden
from monoport_amd import synthetic as syn
from test_octree_select_gpu import ORDERS, order  # noqa: F401  (order: the list-order fixture of that file)
from test_query_gpu import TOL_ORACLE, TOL_REF, _tuned

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
G_CASES = [n for n, c in rc.ALL_QUERY_CASES.items() if c["kind"] == "G" and c["camera"] != "persp"]


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def golden():
    return load_golden(rc.FIXTURE)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


_CASES, _ORACLE = {}, {}


def case(ops, golden, name):
    """The inputs of a query case on the host and on the device (built once): the reference's calibration where
    the fixture has the case, the rebuilt one (equal, tests/test_rect_maps_cpu.py) elsewhere."""
    if name not in _CASES:
        kind, layers, f, p = rc.query_inputs(name)
        calib = golden[name + "_calib"] if name in rc.QUERY_CASES else rc.case_camera(name)
        camera = rc.ALL_QUERY_CASES[name]["camera"]
        from oracle import pifu_oracle as orc
        orc.build()
        xyz = rc.project(orc, p, calib[0], camera)
        _CASES[name] = dict(
            name=name, kind=kind, layers=layers, f=f, p=p, calib=calib, camera=camera,
            projection="perspective" if camera == "persp" else "orthogonal",
            ref=golden[name] if name in rc.QUERY_CASES else None,
            inside=rc.inside_image(xyz), outside=rc.outside_image(xyz), nan=~np.isfinite(xyz[:2]).all(0),
            mlp=ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP[kind]),
            fh=ops.pack_features(dev(f)[None]), pts=dev(p)[None], cal=dev(calib))
        assert _CASES[name]["inside"].sum() >= rc.MIN_INSIDE and _CASES[name]["outside"].sum() >= rc.MIN_OUTSIDE
    return _CASES[name]


def oracle_out(oracle, c, precision, head="own", swapped=None):
    """oracle.query of a case (cached): ``head`` "own" or "three" (rc.three_output_head, tanh); ``swapped``: on one
    of rc.swapped_maps instead of the map."""
    key = (c["name"], precision, head, swapped)
    if key not in _ORACLE:
        layers = c["layers"] if head == "own" else rc.three_output_head(c["layers"])
        f = c["f"] if swapped is None else rc.swapped_maps(c["f"])[swapped]
        out = rc.oracle_query(oracle, c["name"], f, c["p"], c["calib"][0], layers, precision,
                              last_op=None if head == "own" else 2)
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def far_from_exchanged(oracle, c, out, bar, head="own", precision="f32"):
    """Section "independence from the yardstick": the kernel's output is more than 100 bars away from the oracle
    on the maps an exchanged (h, w) would read."""
    ok = ~c["nan"]
    far = {k: float(np.abs(out - oracle_out(oracle, c, precision, head, k))[:, ok].max()) for k in ("transposed", "reread")}
    assert min(far.values()) > 100 * bar, far
    return far


def run_query(ops, c, mlp=None, n=None, mode=None, pts=None):
    """ops.query of a case under its projection -> [Cout,n] numpy; ``mode``: mp_query_tune while it runs."""
    pts = c["pts"] if pts is None else pts
    if n is not None:
        pts = pts[:, :, :n].contiguous()
    mlp = c["mlp"] if mlp is None else mlp
    if mode is None:
        return ops.query(mlp, c["fh"], pts, c["cal"], syn.Z_SCALE, c["projection"])[0].cpu().numpy()
    with _tuned(mode):
        return ops.query(mlp, c["fh"], pts, c["cal"], syn.Z_SCALE, c["projection"])[0].cpu().numpy()


def same(a, b):
    """array_equal with NaN equal to NaN (the z_cam == 0 points under perspective)."""
    return np.array_equal(a, b, equal_nan=True)


# ---- ops.index -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.INDEX_CASES))
def test_index(ops, oracle, golden, name):
    f, uv = rc.index_inputs(name)
    out = ops.index(ops.pack_features(dev(f)[None]), dev(uv)[None])[0].cpu().numpy()
    assert np.array_equal(out, golden[name])  # the reference's own FMA chain: identical bits
    assert np.array_equal(out, oracle.sample(f, uv, precision="f32"))
    for k, g in rc.swapped_maps(f).items():
        assert np.abs(oracle.sample(g, uv, precision="f32") - out).max() > 1.0, k


# ---- the plain f32 kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rc.ALL_QUERY_CASES))
def test_plain_kernel(ops, oracle, golden, name):
    """pifu_query_kernel<C, Cout> (64-point tiles) and its 32-point form: the bars of tests/test_query_gpu.py:
    test_query_vs_reference_golden_and_oracle, ragged prefixes and a permuted [1,N,3] view of the points."""
    c = case(ops, golden, name)
    ok = ~c["nan"]
    out = run_query(ops, c, mode=0)
    assert out.shape == (c["mlp"].cout, rc.N_POINTS)
    assert np.array_equal(np.isnan(out).all(0), c["nan"]) and np.isfinite(out[:, ok]).all()
    ref32, ref64 = oracle_out(oracle, c, "f32"), oracle_out(oracle, c, "f64")
    e32, e64 = float(np.abs(out - ref32)[:, ok].max()), float(np.abs(out - ref64)[:, ok].max())
    line = "%s: |gpu - f32 oracle| %.3g (bar %.0e), |gpu - f64| %.3g" % (name, e32, 3 * TOL_ORACLE, e64)
    if c["ref"] is not None:
        assert np.array_equal(np.isnan(c["ref"]).all(0), c["nan"])  # NaN exactly where the reference has NaN
        e_ref, err_ref = float(np.abs(out - c["ref"])[:, ok].max()), float(np.abs(c["ref"] - ref64)[:, ok].max())
        line += ", |gpu - reference| %.3g (bar %.0e), |reference - f64| %.3g" % (e_ref, TOL_REF, err_ref)
    far = far_from_exchanged(oracle, c, out, 3 * TOL_ORACLE)
    print(line + "; on the exchanged maps %s" % far)
    assert e32 <= 3 * TOL_ORACLE
    if c["ref"] is not None:
        assert e_ref <= TOL_REF and e64 <= max(2 * err_ref, 1e-5)  # no noisier than the reference
    assert (out[:, c["outside"]] == 0).all() and (np.abs(out[:, c["inside"]]) > 0).all()
    # the 32-point kernel and the default gate: the same bits
    assert same(run_query(ops, c, mode=1), out) and same(run_query(ops, c), out)
    for mode in (0, 1):
        for n in (1, 31, 33, 65, 1000):
            assert same(run_query(ops, c, n=n, mode=mode), out[:, :n]), (mode, n)
    pts_n3 = c["pts"].permute(0, 2, 1).contiguous()  # [1,N,3], what query_func hands the net
    assert same(run_query(ops, c, pts=pts_n3.permute(0, 2, 1), mode=0), out)


@pytest.mark.parametrize("name", G_CASES)
def test_plain_kernel_three_outputs(ops, oracle, golden, name):
    """The C = 256, Cout = 3 instantiation: a 3-channel tanh head on the case's 256-channel map."""
    c = case(ops, golden, name)
    mlp3 = ops.PackedMLP.from_layers(DEV, rc.three_output_head(c["layers"]), 2)
    out = run_query(ops, c, mlp3, mode=0)
    ref = oracle_out(oracle, c, "f32", "three")
    err = float(np.abs(out - ref).max())
    print("%s Cout = 3: |gpu - f32 oracle| %.3g (bar %.0e)" % (name, err, 3 * TOL_ORACLE))
    assert out.shape == (3, rc.N_POINTS) and err <= 3 * TOL_ORACLE
    assert (out[:, c["outside"]] == 0).all()
    assert np.array_equal(run_query(ops, c, mlp3, mode=1), out)
    for n in (1, 31, 33, 65, 1000):
        assert np.array_equal(run_query(ops, c, mlp3, n=n, mode=1), out[:, :n]), n


# ---- the skip table --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout", [1, 3])
@pytest.mark.parametrize("name", G_CASES)
def test_skip_table_contents_and_query(ops, oracle, golden, name, cout):
    """mp_skip_table on a non-square map against float64 products (tests/test_query_gpu.py:
    test_skip_table_matches_float64_products), and the f32 query through it (pifu_query_tabws_kernel<Cout>) at the
    bars of test_three_output_head_through_the_skip_table / test_skip_table_ragged_sizes_and_device_counts."""
    c = case(ops, golden, name)
    head = "own" if cout == 1 else "three"
    layers = c["layers"] if cout == 1 else rc.three_output_head(c["layers"])
    mlp = c["mlp"] if cout == 1 else ops.PackedMLP.from_layers(DEV, layers, 2)
    h, w = c["f"].shape[1:]
    plain = run_query(ops, c, mlp)
    try:
        table = ops.skip_table(mlp, c["fh"])
        got = table.table.cpu().numpy()
        out = run_query(ops, c, mlp)
        for n in (1, 31, 33, 1000):
            assert np.array_equal(run_query(ops, c, mlp, n=n), out[:, :n]), n
        n = 1000
        pts = torch.zeros((3, n + 7), device=DEV)
        pts[:, :n] = c["pts"][0, :, :n]
        counted = ops.query_counted(mlp, c["fh"], pts.contiguous(), torch.tensor([n], dtype=torch.int32, device=DEV),
                                    c["cal"], syn.Z_SCALE).cpu().numpy()
    finally:
        ops.skip_table_release(mlp.ctx)
    assert got.shape == (h, w, ops.SKIP_TABLE_ROWS)
    row0, f64 = 0, c["f"].astype(np.float64)
    for l, (wl, _) in enumerate(layers):
        hidden = wl.shape[1] - 257  # input = [hidden | 256 features | z]
        want = np.einsum("rc,chw->hwr", wl[:, hidden:hidden + 256].astype(np.float64), f64)
        assert np.abs(got[:, :, row0:row0 + wl.shape[0]] - want).max() <= 2e-6 * np.abs(want).max(), l
        row0 += wl.shape[0]
    assert row0 == 1920 + cout
    ref = oracle_out(oracle, c, "f32", head)
    d_plain, d_ref = float(np.abs(out - plain).max()), float(np.abs(out - ref).max())
    far = far_from_exchanged(oracle, c, out, TOL_ORACLE, head)
    print("%s Cout = %d through the table: |table - plain| %.3g (bar 2e-6), |table - f32 oracle| %.3g (bar %.0e); on the "
          "exchanged maps %s" % (name, cout, d_plain, d_ref, TOL_ORACLE, far))
    assert not np.array_equal(out, plain)  # the table kernel ran
    assert d_plain <= 2e-6 and d_ref <= TOL_ORACLE
    if cout == 1 and c["ref"] is not None:
        assert np.abs(out - c["ref"]).max() <= TOL_REF
    assert (out[:, c["outside"]] == 0).all()
    assert np.array_equal(counted[:, :n], out[:, :n]) and (counted[:, n:] == 0).all()
    assert np.array_equal(run_query(ops, c, mlp), plain)  # released: the plain path again


def test_registry_refuses_the_other_size(ops, golden):
    """A table registered for a 48 x 80 map must not serve the same buffer viewed as 80 x 48 (find_skip_tables is
    keyed on the address AND (h, w)): that query equals the plain path of an unregistered clone."""
    c = case(ops, golden, "G_wide_scene")
    fh = c["fh"].clone()
    h, w, ch = fh.shape
    other = fh.view(w, h, ch)
    q = lambda m: ops.query(c["mlp"], m, c["pts"], c["cal"], syn.Z_SCALE)
    plain, plain_other = q(fh.clone()), q(other.clone())
    assert not torch.equal(plain, plain_other)
    try:
        table = ops.skip_table(c["mlp"], fh)
        through, got_other = q(fh), q(other)
    finally:
        ops.skip_table_release(c["mlp"].ctx)
    assert not torch.equal(through, plain) and float((through - plain).abs().max()) <= 2e-6
    assert torch.equal(got_other, plain_other)
    assert torch.equal(q(fh), plain) and torch.equal(q(other), plain_other)
    del table


# ---- the f16 kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,tol64", [("f16x3", 2e-5), ("f16w", 3e-4), ("f16", 5e-3)])
@pytest.mark.parametrize("name", ["G_wide_scene", "G_tall_eye"])
def test_f16_kernels_plain_and_through_the_table(ops, oracle, golden, name, precision, tol64, monkeypatch):
    """pifu_query16_kernel and pifu_query16_tab_kernel: f16x3 at 2e-5 to float64 (test_f16x3_ragged_sizes_and_large_
    weights) and the f32 bars of test_f16x3_query_is_f32_class, f16w / f16 at 3e-4 / 5e-3 (test_fp16_modes_report_
    error); through the table as test_f16_kernels_through_the_skip_table; ragged tails of the 96-point tile."""
    monkeypatch.setenv("MONOPORT_TAB16", "all")
    c = case(ops, golden, name)
    mlp = ops.PackedMLP.from_layers(DEV, c["layers"], 1)
    ref64 = oracle_out(oracle, c, "f64")
    plain32 = run_query(ops, c, mlp)
    mlp.set_precision(precision)
    plain16 = run_query(ops, c, mlp)
    for n in (1, 95, 96, 97, 1000):
        assert np.array_equal(run_query(ops, c, mlp, n=n), plain16[:, :n]), n
    try:
        table = ops.skip_table(mlp, c["fh"])
        out = run_query(ops, c, mlp)
        for n in (1, 95, 96, 97, 1000):
            assert np.array_equal(run_query(ops, c, mlp, n=n), out[:, :n]), n
        mlp.set_precision("f32")
        tab32 = run_query(ops, c, mlp)
    finally:
        ops.skip_table_release(mlp.ctx)
    err_plain, err, err_ref = (float(np.abs(v - ref64).max()) for v in (plain16, out, c["ref"]))
    far = far_from_exchanged(oracle, c, plain16, tol64, precision="f64")
    far_from_exchanged(oracle, c, out, tol64, precision="f64")
    print("%s %s: |plain - f64| %.3g, |table - f64| %.3g (bar %.0e; reference %.3g), |plain - f32 kernel| %.3g, "
          "|table - f32 table| %.3g; on the exchanged maps %s"
          % (name, precision, err_plain, err, tol64, err_ref, np.abs(plain16 - plain32).max(), np.abs(out - tab32).max(), far))
    assert np.isfinite(plain16).all() and np.isfinite(out).all()
    assert not np.array_equal(plain16, plain32) and not np.array_equal(out, plain16)  # the f16 and the table kernels ran
    assert err_plain <= tol64
    if precision == "f16x3":
        assert np.abs(plain16 - c["ref"]).max() <= TOL_REF and np.abs(out - c["ref"]).max() <= TOL_REF
        assert err_plain <= max(2 * err_ref, 1e-5) and np.abs(plain16 - plain32).max() <= 2e-6
        assert err <= max(2 * err_ref, 1e-5) and np.abs(out - tab32).max() <= 2e-6
    else:
        assert err <= tol64 and err <= 1.5 * err_plain + 1e-6
    assert (plain16[:, c["outside"]] == 0).all() and (out[:, c["outside"]] == 0).all()
    del table


# ---- the batched and counted forms ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", [False, True])
def test_batched_forms_equal_single_frames(ops, golden, tables):
    """mp_query_batch / mp_query_counted_batch_proj: three frames of distinct 48 x 80 maps, mixed projections, device
    counts [4096, 0, 977], under every tile gate: each row is the single-frame call bit for bit."""
    c = case(ops, golden, "G_wide_scene")
    h, w = rc.SHAPES["wide"]
    mlp = c["mlp"]
    feats = [ops.pack_features(dev(syn.rand_feat(256, h, w, 680 + i))[None]) for i in range(3)]
    pts = torch.stack([dev(rc.rect_points(h, w, 690 + i)) for i in range(3)])
    cals = [c["cal"], dev(rc.persp_calib()), torch.eye(4, device=DEV)[None]]
    proj = ["orthogonal", "perspective", "orthogonal"]
    counts_host = [4096, 0, 977]
    counts = [torch.tensor([k], dtype=torch.int32, device=DEV) for k in counts_host]
    runs = {}
    with registered(ops, mlp, feats, tables):
        for mode in (0, 1, -1):
            with _tuned(mode):
                single = [ops.query(mlp, feats[i], pts[i:i + 1], cals[i], syn.Z_SCALE, proj[i])[0] for i in range(3)]
                batch = ops.query_batch(mlp, feats, pts, cals, proj, syn.Z_SCALE)
                counted = ops.query_counted_batch(mlp, feats, [p.contiguous() for p in pts], counts, cals, syn.Z_SCALE,
                                                  projections=proj)
                ortho = ops.query_counted(mlp, feats[2], pts[2].contiguous(), counts[2], cals[2], syn.Z_SCALE)
            for i, k in enumerate(counts_host):
                assert not torch.isnan(single[i]).any() and float(single[i].abs().max()) > 0
                assert torch.equal(batch[i], single[i]), (mode, i)
                assert torch.equal(counted[i][:, :k], single[i][:, :k]), (mode, i)
                assert float(counted[i][:, k:].abs().max()) == 0.0 if k < rc.N_POINTS else True
            assert torch.equal(ortho, counted[2])
            runs[mode] = single
    if tables:  # the tables were read
        plain = ops.query(mlp, feats[0], pts[0:1], cals[0], syn.Z_SCALE)[0]
        assert not torch.equal(plain, runs[0][0]) and float((plain - runs[0][0]).abs().max()) <= 2e-6
    else:  # the 64- and the 32-point plain kernels: one set of bits
        assert all(torch.equal(a, b) for m in (1, -1) for a, b in zip(runs[0], runs[m]))


# ---- the multi-view kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,shape,v_n", [("G", "wide", 3), ("C", "tall", 2)])
def test_query_views(ops, oracle, kind, shape, v_n):
    """mp_query_views against the float64 model of tests/test_query_views_gpu.py (ops.index samples, held to the
    reference bit for bit by test_index above) at its bar; one view equals the plain query."""
    import test_query_views_gpu as tv
    h, w = rc.SHAPES[shape]
    ch = syn.MLP_DIMS[kind][0] - 1
    layers = syn.rand_mlp(kind, 720 + v_n, 2.0)
    mlp = ops.PackedMLP.from_layers(DEV, layers, syn.LAST_OP[kind])
    maps = [syn.rand_feat(ch, h, w, 730 + v) for v in range(v_n)]
    fh = [ops.pack_features(dev(m)[None]) for m in maps]
    calibs = dev(np.stack([oracle.pifu_calib(*syn.scene_camera(37 * v))[0] for v in range(v_n)]))
    pts = torch.stack([dev(rc.rect_points(h, w, 740 + v)) for v in range(v_n)])
    out = ops.query_views(mlp, fh, pts, calibs, "orthogonal", syn.Z_SCALE).cpu().numpy()
    ref = tv.model_views(ops, layers, fh, pts, calibs, syn.LAST_OP[kind])
    err = float(np.abs(out - ref).max())
    # the model on the maps an exchanged (h, w) would read: the same buffers viewed [W,H,C], and the transposed maps
    far = {"reread": float(np.abs(out - tv.model_views(ops, layers, [m.view(w, h, ch) for m in fh], pts, calibs,
                                                       syn.LAST_OP[kind])).max()),
           "transposed": float(np.abs(out - tv.model_views(
               ops, layers, [ops.pack_features(dev(m.transpose(0, 2, 1))[None]) for m in maps], pts, calibs,
               syn.LAST_OP[kind])).max())}
    print("views %s V = %d on %d x %d: max |d| vs float64 = %.3g (bar %.0e); on the exchanged maps %s"
          % (kind, v_n, h, w, err, tv.TOL_MODEL, far))
    assert out.shape == (v_n, mlp.cout, rc.N_POINTS) and err <= tv.TOL_MODEL
    assert min(far.values()) > 100 * tv.TOL_MODEL
    assert (out == 0).all(1).sum() >= rc.MIN_OUTSIDE and (out != 0).all(1).sum() >= rc.MIN_INSIDE
    one = ops.query_views(mlp, fh[:1], pts[:1], calibs[:1], "orthogonal", syn.Z_SCALE)
    for gate in (0, 1):
        with _tuned(gate):
            assert torch.equal(one, ops.query(mlp, fh[0], pts[:1], calibs[0], syn.Z_SCALE))


# ---- fused reconstruction -------------------------------------------------------------------------------------------
_SCENES, _CPU_FIELD = {}, {}


def scene(ops, oracle, shape):
    """A reconstruction case on the device (tests/test_recon_gpu.py's ``body`` on a non-square map)."""
    if shape not in _SCENES:
        layers, f = rc.recon_inputs(shape)
        calib = oracle.pifu_calib(*syn.scene_camera(rc.RECON_STEP))
        mlp = ops.PackedMLP.from_layers(DEV, layers, 1)
        fh, cal = ops.pack_features(dev(f)[None]), dev(calib)

        def gpu_query(pts):  # [3,N] numpy -> [N] numpy through the HIP kernel (through the table while one is registered)
            return ops.query(mlp, fh, dev(pts)[None], cal, syn.Z_SCALE)[0, 0].cpu().numpy()

        _SCENES[shape] = dict(layers=layers, f=f, calib=calib, mlp=mlp, fh=fh, cal=cal, gpu_query=gpu_query)
    return _SCENES[shape]


def cpu_field(oracle, shape):
    if shape not in _CPU_FIELD:
        s = _SCENES[shape]
        stats = []
        vol = oracle.seg3d_lossless(
            lambda p: oracle.query(s["f"], p, s["calib"][0], s["layers"], 1, syn.Z_SCALE, precision="f32")[0],
            BMIN, BMAX, rc.RECON_RES, stats=stats)
        vol.setflags(write=False)
        _CPU_FIELD[shape] = (vol, stats)
    return _CPU_FIELD[shape]


class registered:
    """with registered(ops, mlp, maps, on): the maps' skip tables exist inside the block when ``on``."""

    def __init__(self, ops, mlp, maps, on):
        self.ops, self.mlp, self.maps, self.on, self.handles = ops, mlp, maps, on, []

    def __enter__(self):
        if self.on:
            self.handles = [self.ops.skip_table(self.mlp, m) for m in self.maps]

    def __exit__(self, *exc):
        for t in self.handles:
            t.release()


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("shape", ["wide", "tall"])
def test_recon(ops, oracle, shape, table, order):
    """ops.recon: the decisions of the CPU restatement driven by the same HIP query (test_recon_bit_exact_vs_oracle_
    driver), and against the all-CPU field (test_recon_matches_cpu_oracle_field) with the share of nodes the margin
    leaves out bounded by 0.1 %."""
    s = scene(ops, oracle, shape)
    with registered(ops, s["mlp"], [s["fh"]], table):
        vol, status = ops.recon(s["mlp"], s["fh"], s["cal"], syn.Z_SCALE, BMIN, BMAX, rc.RECON_RES)
        stats = []
        ref = oracle.seg3d_lossless(s["gpu_query"], BMIN, BMAX, rc.RECON_RES, stats=stats)
    v, status = vol.cpu().numpy(), status.cpu().numpy().tolist()
    cpu, cpu_stats = cpu_field(oracle, shape)
    safe = np.abs(cpu - 0.5) > 1e-3
    err, left_out = float(np.abs(v - cpu).max()), float(1 - safe.mean())
    print("recon %s table %s order %s: status %s, |gpu - cpu field| %.3g (bar 1e-4), %.4f %% of the nodes within 1e-3 of "
          "the threshold" % (shape, table, order, status, err, 100 * left_out))
    assert status[0] == 1 and status[1:] == stats
    assert np.array_equal(v, ref)
    assert cpu_stats == rc.RECON_COUNTS[shape]
    if not table:
        assert status[1:] == rc.RECON_COUNTS[shape]
    assert err <= 1e-4 and left_out <= 1e-3
    assert np.array_equal((v > 0.5)[safe], (cpu > 0.5)[safe])
    # the other map's field is another body: the volume tells the two apart
    other = "tall" if shape == "wide" else "wide"
    scene(ops, oracle, other)
    assert ((v > 0.5) != (cpu_field(oracle, other)[0] > 0.5)).sum() > 0


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("table", [False, True])
def test_recon_batch_equals_single_frames(ops, oracle, table, order):
    """Three 48 x 80 maps (seeds 2, 3, 4), the middle frame's camera looking past the box (an empty frame); then the
    three maps under body_mlp(c=-3.0), empty everywhere: every live frame equals its single-frame call bit for bit,
    every empty one has the status [0, 9^3, 0, 0, 0]."""
    s = scene(ops, oracle, "wide")
    h, w = rc.SHAPES["wide"]
    feats = [s["fh"]] + [ops.pack_features(dev(syn.body_feat(256, h, w, seed))[None]) for seed in (3, 4)]
    cals = []
    for i in range(3):
        calib = oracle.pifu_calib(*syn.scene_camera(rc.RECON_STEP + 25 * i))
        if i == 1:
            calib[0, 0, 3] = 5.0
        cals.append(dev(calib))
    empty_status = [0, rc.RECON_RES[0] ** 3] + [0] * (len(rc.RECON_RES) - 1)
    for mlp, live in ((s["mlp"], [True, False, True]),
                      (ops.PackedMLP.from_layers(DEV, syn.body_mlp("G", c=-3.0), 1), [False] * 3)):
        with registered(ops, mlp, feats, table):
            vols, status = ops.recon_batch(mlp, feats, cals, syn.Z_SCALE, BMIN, BMAX, rc.RECON_RES)
            single = [ops.recon(mlp, feats[i], cals[i], syn.Z_SCALE, BMIN, BMAX, rc.RECON_RES) for i in range(3)]
        status = status.cpu().tolist()
        print("recon_batch table %s order %s: status %s" % (table, order, status))
        for i in range(3):
            assert status[i] == single[i][1].cpu().tolist(), i
            if live[i]:
                assert status[i][0] == 1 and torch.equal(vols[i], single[i][0]), i
            else:
                assert status[i] == empty_status, i
    assert not torch.equal(single[0][0], single[2][0])


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("table", [False, True])
def test_recon_batch_perspective_equals_generic_engine(ops, oracle, table, order):
    """One perspective frame through recon_batch(projections=...) equals the level-at-a-time engine driven by
    ops.query(..., "perspective") on the same 48 x 80 map."""
    from test_query_batch_persp_gpu import persp_body_mlp
    from test_recon_views_gpu import same_bits
    h, w = rc.SHAPES["wide"]
    mlp = ops.PackedMLP.from_layers(DEV, persp_body_mlp("G", 751, 0.05), 1)
    fh = ops.pack_features(dev(syn.body_feat(256, h, w, 752))[None])
    cal = dev(rc.persp_calib(focal=2.0))  # the body of persp_body_mlp sits at the depth of this camera, in its image

    def query_func(points):  # [1,N,3] -> [1,1,N]
        return ops.query(mlp, fh, points.permute(0, 2, 1), cal, syn.Z_SCALE, "perspective")

    with registered(ops, mlp, [fh], table):
        vols, status = ops.recon_batch(mlp, [fh], [cal], syn.Z_SCALE, BMIN, BMAX, rc.RECON_RES,
                                       projections=["perspective"])
        gen, counts = ops.recon_generic(query_func, {}, DEV, BMIN, BMAX, rc.RECON_RES)
    status = status.cpu().tolist()[0]
    inside = float((vols[0] > 0.5).float().mean())
    print("perspective recon on %d x %d: status %s, generic counts %s, inside %.4f" % (h, w, status, counts, inside))
    assert gen is not None and status == [1] + counts and 0.005 < inside < 0.5
    assert same_bits(vols[0], gen)


@pytest.mark.parametrize("order", ORDERS, indirect=True)
def test_recon_views_equals_generic_engine(ops, oracle, order):
    """mp_recon_views, V = 2 on 80 x 48 maps: the fused engine equals the level-at-a-time engine bit for bit
    (tests/test_recon_views_gpu.py: test_fused_equals_generic_bitwise)."""
    import test_query_views_gpu as tv
    import test_recon_views_gpu as rv
    h, w = rc.SHAPES["tall"]
    v_n = 2
    net = tv._net("G", syn.body_mlp("G", noise=0.05, seed=251), v_n)
    maps = np.stack([syn.body_feat(256, h, w, 252 + v) for v in range(v_n)])
    feats = [[torch.zeros(v_n, 256, 2, 2, device=DEV)]] * 3 + [[dev(maps)]]
    calib = dev(tv.calibs_of(dict(proj="orthogonal", steps=[6 * v for v in range(v_n)])))
    ef, vf, eg, vg = rv.fused_and_generic(net, v_n, feats, calib, rc.RECON_RES)
    sf, sg = ef.last_status.tolist(), eg.last_status.tolist()
    print("recon_views on %d x %d: status fused %s generic %s, inside %.4f" % (h, w, sf, sg, float((vf > 0.5).float().mean())))
    assert vf is not None and vg is not None and bool((vf > 0.5).any()) and bool((vf < 0.5).any())
    assert sf == sg and sf[-1] > 0 and torch.equal(vf, vg)


@pytest.mark.parametrize("order", ORDERS, indirect=True)
@pytest.mark.parametrize("table", [False, True])
def test_recon_topk_bit_exact_vs_restatement(ops, oracle, table, order):
    """ops.recon_topk on the 48 x 80 map against tests/topk_ref.py driven by the same HIP query: budgets of a quarter
    of the lossless counts and one above them (tests/test_topk_gpu.py: test_recon_topk_bit_exact_vs_restatement)."""
    from test_topk_gpu import _check_fused
    s = scene(ops, oracle, "wide")
    res = rc.RECON_RES
    lossless = rc.RECON_COUNTS["wide"]
    quarter = [0] + [max(k // 4, 1) for k in lossless[1:]]
    above = [0] + [min(2 * k, r ** 3) for k, r in zip(lossless[1:], res[1:])]
    with registered(ops, s["mlp"], [s["fh"]], table):
        _, stats = _check_fused(ops, s, res, quarter)
        assert stats[1:] == quarter[1:]
        _check_fused(ops, s, res, above)


# ---- the Python layer ------------------------------------------------------------------------------------------------
def _single_view_net(kind, layers):
    import test_query_views_gpu as tv
    return tv._net(kind, layers, 1)


def test_monoportnet_query_and_engine(ops, oracle, golden):
    """PIFuNetG.query on a stage list whose last map is [1,256,48,80] equals ops.query on pack_features of it, and
    Seg3dLossless driven by that net's query_func returns the volume of ops.recon through the map's skip table."""
    from monoport_amd.implicit_seg.functional import Seg3dLossless
    c = case(ops, golden, "G_wide_scene")
    s = scene(ops, oracle, "wide")
    net = _single_view_net("G", s["layers"])
    f = dev(s["f"])[None]
    feats = [[torch.zeros(1, 256, 2, 2, device=DEV)]] * 3 + [[f]]
    assert tuple(f.shape) == (1, 256, 48, 80)
    with torch.no_grad():
        out = net.query(feats, c["pts"], s["cal"])[0]
    assert torch.equal(out, ops.query(s["mlp"], ops.pack_features(f), c["pts"], s["cal"], syn.Z_SCALE))
    assert bool((out == 0).any()) and bool((out > 0).any())

    def query_func(points, im_feat_list, calib_tensor):  # RTL/main.py:169-183
        return net.query(im_feat_list, points=points.permute(0, 2, 1), calibs=calib_tensor)[0]

    eng = Seg3dLossless(query_func=query_func, b_min=np.array([BMIN]), b_max=np.array([BMAX]),
                        resolutions=rc.RECON_RES, balance_value=0.5, faster=True).to(DEV)
    with torch.no_grad():
        vol = eng(im_feat_list=feats, calib_tensor=s["cal"])
    assert eng.last_path == "fused" and net.has_skip_table()
    with registered(ops, s["mlp"], [s["fh"]], True):
        want, status = ops.recon(s["mlp"], s["fh"], s["cal"], syn.Z_SCALE, BMIN, BMAX, rc.RECON_RES)
    assert eng.last_status.tolist() == status.cpu().tolist()
    assert torch.equal(vol[0, 0], want)


def test_vertex_colours_on_a_tall_map(ops, oracle):
    """mesh_util.vertex_colors and recon.reconstruct_mesh(netC=...) with a [1,512,80,48] colour map on the marching-
    cubes mesh of the 80 x 48 reconstruction: the same bits, within TOL_ORACLE of oracle.query at the vertices."""
    from monoport_amd import mesh_util
    from monoport_amd.recon import marching_cubes, reconstruct_mesh
    s = scene(ops, oracle, "tall")
    h, w = rc.SHAPES["tall"]
    vol, status = ops.recon(s["mlp"], s["fh"], s["cal"], syn.Z_SCALE, BMIN, BMAX, rc.RECON_RES)
    layers = syn.rand_mlp("C", 761, 2.0)
    net = _single_view_net("C", layers)
    fc = syn.rand_feat(512, h, w, 762)
    feat_c = [[dev(fc)[None]]]
    assert tuple(feat_c[0][0].shape) == (1, 512, 80, 48)
    verts, faces = marching_cubes(vol[None, None], 0.5, BMIN, BMAX)
    mesh = reconstruct_mesh(vol[None, None], 0.5, BMIN, BMAX, netC=net, feat_tensor_C=feat_c, calib_tensor=s["cal"])
    colors = mesh_util.vertex_colors(net, feat_c, verts, s["cal"])
    assert verts.shape[0] > 1000 and torch.equal(mesh.verts, verts) and torch.equal(mesh.faces, faces)
    assert torch.equal(mesh.colors, colors)
    v = verts.cpu().numpy()
    ref = oracle.query(fc, np.ascontiguousarray(v.T), s["calib"][0], layers, 2, syn.Z_SCALE, precision="f32")
    pred = (colors.cpu().numpy().astype(np.float64).T - 0.5) * 2  # colour = prediction * 0.5 + 0.5
    err = float(np.abs(pred - ref).max())
    far = {k: float(np.abs(pred - oracle.query(g, np.ascontiguousarray(v.T), s["calib"][0], layers, 2, syn.Z_SCALE,
                                                precision="f32")).max()) for k, g in rc.swapped_maps(fc).items()}
    print("colours of %d vertices on a %d x %d map: |gpu - f32 oracle| %.3g (bar %.0e); on the exchanged maps %s"
          % (v.shape[0], h, w, err, TOL_ORACLE, far))
    assert err <= TOL_ORACLE and min(far.values()) > 100 * TOL_ORACLE
    assert (ref != 0).all(0).mean() > 0.9  # the body's vertices are in the image
