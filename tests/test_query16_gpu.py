"""The f16 query kernels (csrc/query16.hip: f16x3 / f16w / f16, Cout 1 / 3, plain and skip-table)
against the float64 model of their own arithmetic (oracle/split_precision.py), at the bars fixed on the
CPU in tests/test_split_precision_cpu.py.  Needs an MI355X."""
import numpy as np
import pytest

from monoport_amd import synthetic as syn
from test_split_precision_cpu import (BAR, BAR_MEDIAN, N_SWEEP, PRECISIONS, range_case, sweep_case, syn_calib)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops as _ops
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _ops


@pytest.fixture(scope="module")
def sp(oracle):
    from oracle import split_precision
    return split_precision


_MODEL = {}


def _model(sp, key, case, precision, table):
    k = (key, precision, table)
    if k not in _MODEL:
        layers, last_op, feat, pts, calib = case
        _MODEL[k] = sp.query_emulated(feat, pts, calib, layers, last_op, syn.Z_SCALE, precision, table=table)
    return _MODEL[k]


class Head:
    """One head + feature map on the device, queried on the plain kernel or through the skip table."""

    def __init__(self, ops, case, precision):
        self.ops = ops
        layers, last_op, feat, _, calib = case
        self.mlp = ops.PackedMLP.from_layers(DEV, layers, last_op)
        self.mlp.set_precision(precision)
        self.fh = ops.pack_features(torch.from_numpy(feat)[None].to(DEV))
        self.cal = torch.from_numpy(np.asarray(calib)[None]).to(DEV)

    def query(self, pts, table, monkeypatch):
        """pts: [1,3,N] device tensor (any strides) -> [Cout, N] numpy."""
        monkeypatch.setenv("MONOPORT_TAB16", "all" if table else "off")
        if not table:
            return self.ops.query(self.mlp, self.fh, pts, self.cal, syn.Z_SCALE)[0].cpu().numpy()
        handle = None
        try:
            handle = self.ops.skip_table(self.mlp, self.fh)
            return self.ops.query(self.mlp, self.fh, pts, self.cal, syn.Z_SCALE)[0].cpu().numpy()
        finally:
            self.ops.skip_table_release(self.mlp.ctx)
            del handle


def _outside(oracle, pts, calib):
    xyz = oracle.orthogonal(pts, calib)
    return (np.abs(xyz[0]) > 1) | (np.abs(xyz[1]) > 1)


def _check(out, model, precision, cout, what, median=True):
    """max and (on a few hundred points or more) median of |kernel - model| against the bars."""
    d = np.abs(out.astype(np.float64) - model)
    print("%s: max|kernel - model| %.3g (bar %.3g), median %.3g (bar %.3g)"
          % (what, d.max(), BAR[precision, cout], np.median(d), BAR_MEDIAN[precision, cout]))
    assert np.isfinite(out).all()
    assert d.max() <= BAR[precision, cout], what
    if median:
        assert np.median(d) <= BAR_MEDIAN[precision, cout], what


@pytest.mark.parametrize("head", ["rand", "body"])
@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
@pytest.mark.parametrize("cout", [1, 3])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_instantiation_against_the_model(ops, oracle, sp, monkeypatch, precision, cout, table, head):
    """All twelve kernels {f16x3, f16w, f16} x Cout {1, 3} x {pifu_query16_kernel, pifu_query16_tab_kernel},
    on a random and a body head; out-of-image points exactly 0."""
    case = sweep_case(head, cout)
    h = Head(ops, case, precision)
    pts = case[3]
    out = h.query(torch.from_numpy(pts)[None].to(DEV), table, monkeypatch)
    assert out.shape == (cout, N_SWEEP)
    outside = _outside(oracle, pts, case[4])
    assert outside.any() and (out[:, outside] == 0).all()
    _check(out, _model(sp, (head, cout), case, precision, table), precision, cout,
           "%s Cout %d %s %s head" % (precision, cout, "table" if table else "plain", head))


@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
@pytest.mark.parametrize("precision", ["f16w", "f16"])
def test_tile_edges_and_strided_points(ops, sp, monkeypatch, precision, table):
    """Ragged launches around the 96-point tile (n = 1, 95 .. 97, 191 .. 193, 1000): each against the
    model and bit-identical to the same points of the full launch; a strided [N,3]-transposed view too."""
    case = sweep_case("rand", 1)
    h = Head(ops, case, precision)
    pts = torch.from_numpy(case[3])[None].to(DEV)
    full = h.query(pts, table, monkeypatch)
    model = _model(sp, ("rand", 1), case, precision, table)
    for n in (1, 95, 96, 97, 191, 192, 193, 1000):
        part = h.query(pts[:, :, :n].contiguous(), table, monkeypatch)
        assert part.shape == (1, n) and np.array_equal(part, full[:, :n]), n
        _check(part, model[:, :n], precision, 1, "%s %s n = %d" % (precision, "table" if table else "plain", n),
               median=False)
    strided = pts[0].t().contiguous().t()[None]  # [1,3,N] with strides (1, 3)
    assert strided.stride(2) == 3
    assert np.array_equal(h.query(strided, table, monkeypatch), full)
    every_other = torch.stack([pts[0], pts[0]], 2).reshape(1, 3, -1)[:, :, ::2]  # stride 2 along N
    assert np.array_equal(h.query(every_other, table, monkeypatch), full)


@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_weight_range_head_against_the_model(ops, oracle, sp, monkeypatch, precision, table):
    """range_head(): a layer spanning 1e-3 .. 40, a power-of-two max|W| and a layer of ~1e-6 weights
    (S clamped) -- against the model, not only the fp64 oracle."""
    case = range_case()
    h = Head(ops, case, precision)
    out = h.query(torch.from_numpy(case[3])[None].to(DEV), table, monkeypatch)
    _check(out, _model(sp, "range", case, precision, table), precision, 1,
           "weight range %s %s" % (precision, "table" if table else "plain"))
    assert (out[:, _outside(oracle, case[3], case[4])] == 0).all()


@pytest.mark.parametrize("precision", ["f16w", "f16"])
def test_counted_batch_frames_equal_single_frames(ops, oracle, sp, monkeypatch, precision):
    """query_counted_batch with an f16 head: frames of 0, 95, 96, 97 and 5000 points, each with its own
    map and camera, give the bits of their own query_counted call and zeros past the count; the
    5000-point frame against the model on its first N_SWEEP points."""
    monkeypatch.setenv("MONOPORT_TAB16", "off")
    layers, last_op, _, _, _ = sweep_case("rand", 1)
    mlp = ops.PackedMLP.from_layers(DEV, layers, last_op)
    mlp.set_precision(precision)
    counts = [0, 95, 96, 97, 5000]
    cap = 5008
    feats, fhs, pts, cnts, cals = [], [], [], [], []
    for i, n in enumerate(counts):
        feats.append(syn.rand_feat(256, 128, 128, 40 + i))
        fhs.append(ops.pack_features(torch.from_numpy(feats[-1])[None].to(DEV)))
        p = np.zeros((3, cap), np.float32)
        p[:, :n] = syn.rand_points(n, 50 + i, 1.1)
        pts.append(torch.from_numpy(p).to(DEV))
        cnts.append(torch.tensor([n], dtype=torch.int32, device=DEV))
        cals.append(torch.from_numpy(syn_calib(20 * i)[None]).to(DEV))
    outs = ops.query_counted_batch(mlp, fhs, pts, cnts, cals, syn.Z_SCALE)
    for i, n in enumerate(counts):
        single = ops.query_counted(mlp, fhs[i], pts[i], cnts[i], cals[i], syn.Z_SCALE)
        assert torch.equal(outs[i], single), i
        assert float(outs[i][:, n:].abs().max()) == 0.0, i
    p = pts[4][:, :N_SWEEP].cpu().numpy()
    model = sp.query_emulated(feats[4], p, syn_calib(80), layers, last_op, syn.Z_SCALE, precision)
    _check(outs[4][:, :N_SWEEP].cpu().numpy(), model, precision, 1, "%s batch frame 4" % precision)


@pytest.mark.parametrize("table", [False, True], ids=["plain", "table"])
def test_f16w_both_grid_sizes(ops, sp, monkeypatch, table):
    """launch_query16(_tab)_t: host counts (mp_query) get up to 8x the resident grid, device counts
    (mp_query_counted) the resident grid.  200 k points is > 2048 tiles of 96, so both grids walk
    several tiles per workgroup: same bits either way, a subsample against the model."""
    case = sweep_case("rand", 1)
    h = Head(ops, case, "f16w")
    n = 200_000
    p = syn.rand_points(n, 77, 1.1)
    p[:, :N_SWEEP] = case[3]
    pts = torch.from_numpy(p).to(DEV)
    host = h.query(pts[None], table, monkeypatch)
    monkeypatch.setenv("MONOPORT_TAB16", "all" if table else "off")
    cnt = torch.tensor([n], dtype=torch.int32, device=DEV)
    handle = None
    try:
        handle = ops.skip_table(h.mlp, h.fh) if table else None
        dev_counted = ops.query_counted(h.mlp, h.fh, pts, cnt, h.cal, syn.Z_SCALE).cpu().numpy()
    finally:
        ops.skip_table_release(h.mlp.ctx)
        del handle
    assert np.array_equal(host, dev_counted)
    _check(host[:, :N_SWEEP], _model(sp, ("rand", 1), case, "f16w", table), "f16w", 1,
           "f16w %s 200 k points" % ("table" if table else "plain"))
    sub = slice(N_SWEEP + 150_000, N_SWEEP + 150_000 + 960)  # tiles handled in a later pass of the grid loop
    model = sp.query_emulated(case[2], p[:, sub], case[4], case[0], 1, syn.Z_SCALE, "f16w", table=table)
    _check(host[:, sub], model, "f16w", 1, "f16w %s late tiles" % ("table" if table else "plain"))
