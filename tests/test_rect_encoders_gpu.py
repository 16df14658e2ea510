"""Whole encoders on images that are not 512 x 512.  Which path an encoder takes depends on the image size
(HGFilter._dataflow_ok: powers of two, h >= 128, w >= 512; ResnetFilter._dataflow_ok: powers of two, h >= 32,
w >= 256; the per-module kernels below that): every stack's output at five non-square sizes against the float64 copy
of the same module (tests/test_pipeline_slot_gpu.py), at the bar the encoders carry at 512^2, with the path asserted
so that a change of the gates cannot move a case silently.  Needs an MI355X."""
import numpy as np
import pytest

from monoport_amd import synthetic as syn
from test_pipeline_slot_gpu import ENCODER_BAR, nets  # noqa: F401  (nets: that file's encoders and float64 copies)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

# encoder, image height, width, whether the hand-over (dataflow) chain takes it
SIZES = [
    ("hg", 128, 512, True),
    ("hg", 512, 128, False),   # per-module kernels on the large maps, torch operators on the small ones
    ("hg", 384, 320, False),   # not a power of two
    ("res", 64, 256, True),
    ("res", 96, 160, False),
]


def crop(h, w):
    """The centre h x w pixels of synthetic_image(73): [3,h,w] on the device."""
    img = syn.synthetic_image(73)
    y0, x0 = (512 - h) // 2, (512 - w) // 2
    return torch.from_numpy(np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w])).to(DEV)


def stacks(outs):
    return torch.stack([o[0][0] for o in outs])


@pytest.mark.parametrize("which,h,w,dataflow", SIZES)
def test_encoder_vs_float64(nets, monkeypatch, which, h, w, dataflow):  # noqa: F811
    from monoport_amd.modeling import backbones
    netg, netc, ref = nets
    enc, enc64 = (netg.image_filter, ref.g) if which == "hg" else (netc.image_filter, ref.c)
    x = crop(h, w)
    assert float(x.abs().max()) > 0.5 and float((x == 0).float().mean()) > 0.05  # figure and background
    flag = torch.backends.cudnn.deterministic
    with torch.no_grad():
        assert bool(enc._dataflow_ok(x[None])) == dataflow
        out = stacks(enc(x[None], graphed=False))
        again = stacks(enc(x[None], graphed=False))
    want, seconds = ref._run(enc64, x)
    want = stacks(want)
    assert out.shape == want.shape == ((4 if which == "hg" else 1), 256, h // 4, w // 4)
    err = float((out.double() - want).abs().max())
    monkeypatch.setattr(backbones, "ENCODER_CONV", "miopen")
    monkeypatch.setattr(backbones, "ENCODER_DATAFLOW", "off")
    with torch.no_grad():
        stock = stacks(enc(x[None], graphed=False))
    monkeypatch.undo()
    err_stock = float((stock.double() - want).abs().max())
    bar = ENCODER_BAR if err_stock <= ENCODER_BAR else 2 * err_stock
    print("%s %d x %d (%s): vs float64 %.3g (bar %.3g), stock operators %.3g; max |feature| %.3g; float64 pass %.2f s"
          % (type(enc).__name__, h, w, "dataflow" if dataflow else "per-module", err, bar, err_stock,
             float(want.abs().max()), seconds))
    # torch's default Conv2d(128, 64, 3) on the 48 x 40 map of the 384 x 320 case rounded 9 of 10 calls differently: a
    # per-module pass asks for the repeatable solvers while it runs (backbones._repeatable_convs), and only then
    assert torch.equal(out, again), "second pass differs"
    assert torch.backends.cudnn.deterministic == flag
    assert err <= bar


def test_hgfilter_128x512_hwc_output_and_graph(nets):  # noqa: F811
    """At 128 x 512 (the dataflow chain): the channels-last map the producing kernel writes equals pack_features of
    the NCHW output, and the captured graph equals the eager chain, bit for bit."""
    from monoport_amd import ops
    netg, _, _ = nets
    enc = netg.image_filter
    x = crop(128, 512)[None]
    hwc = torch.full((1, 32, 128, 256), float("nan"), device=DEV)
    with torch.no_grad():
        assert enc._dataflow_ok(x)
        eager = stacks(enc(x, graphed=False))
        got = enc(x, last_only=True, hwc_out=hwc, keep_nchw=True, graphed=False)[-1][0]
        graphed = stacks(enc(x, graphed=True))
    assert torch.equal(got, eager[3:4]) and torch.equal(hwc[0], ops.pack_features(got))
    assert torch.equal(graphed, eager)
