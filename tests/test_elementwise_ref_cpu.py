"""The float64 restatements the GPU tests of csrc/encoder_ops.hip compare against (tests/elementwise_ref.py), held to
torch's own float64 CPU ops, and the restated admission rule of the banded upsample kernel held to the lattice.  No GPU.

bicubic2x takes the source coordinate in float32, as torch does for a float32 tensor; F.interpolate on the float64
input takes it in float64.  That rounding alone moves the result by up to 5.4e-6 * max(1, max|ref|) on maps up to 128
on a side (measured on the shapes below), so the two are held to 2e-5 of that scale -- and the GPU kernels, which are
held to 4e-6, are compared with the float32-coordinate form only."""
import numpy as np
import pytest
import torch

import elementwise_ref as er

F = torch.nn.functional


@pytest.mark.parametrize("shape", [(2, 3, 2, 2), (1, 2, 3, 2), (2, 2, 5, 7), (1, 3, 16, 6), (1, 2, 128, 8),
                                   (1, 1, 128, 128), (1, 2, 12, 32), (1, 1, 8, 128)])
def test_bicubic2x_is_torchs_interpolate(shape):
    x = er.values(shape, 3)
    add = er.noise(shape[:2] + (2 * shape[2], 2 * shape[3]), 4)
    want = F.interpolate(x.double(), scale_factor=2, mode="bicubic", align_corners=True)
    scale = max(1.0, want.abs().max().item())
    got = er.bicubic2x(x)
    err = (got - want).abs().max().item() / scale
    print("bicubic2x %s vs float64 interpolate: %.3g of scale %.3g" % (shape, err, scale))
    assert got.dtype == torch.float64 and got.shape == want.shape and err <= 2e-5
    assert torch.equal(er.bicubic2x(x, add), got + add.double())


def test_cubic_weights_are_the_keys_kernel():
    """A = -0.75: the weights sum to one, interpolate at t = 0 and mirror under t -> 1 - t."""
    t = np.linspace(0.0, 1.0, 33)[:-1]
    w = er.cubic_weights(t)
    assert np.abs(w.sum(1) - 1.0).max() <= 1e-15
    assert np.array_equal(w[0], [0.0, 1.0, 0.0, 0.0])
    assert np.abs(w[1:] - w[1:][::-1, ::-1]).max() <= 1e-15
    assert abs(w[16, 0] - (-0.09375)) <= 1e-15 and abs(w[16, 1] - 0.59375) <= 1e-15  # t = 1/2
    assert er.cubic_weights(t.astype(np.float32)).dtype == np.float32


UPSAMPLE_CASES = ([(r[:4], True) for r in er.UPSAMPLE_ROWS] + [(r, False) for r in er.UPSAMPLE_NO_ADD]
                  + [(r, a) for r in er.UPSAMPLE_PLAIN for a in (False, True)])


@pytest.mark.parametrize("shape,with_add", UPSAMPLE_CASES,
                         ids=["%s%s" % ("x".join(map(str, r)), "-add" if a else "") for r, a in UPSAMPLE_CASES])
def test_float32_evaluation_holds_the_gpu_bar(shape, with_add):
    """bicubic2x_at's op order in float32 numpy, every operation rounded on its own (the library is built without FMA
    contraction), against bicubic2x on the data and with the ``add`` the GPU test uses: <= 1e-6 * max(1, max|ref|).
    Measured: <= 8.2e-7 on the rows with ``add``, <= 9.7e-7 without; torch's own float32 CPU kernel <= 6.1e-7.  The
    GPU bar of 4e-6 is therefore held by a correct float32 evaluation alone."""
    x, add = er.upsample_inputs(shape)
    add = add if with_add else None
    ref = er.bicubic2x(x, add)
    scale = max(1.0, ref.abs().max().item())
    model = er.bicubic2x_f32_model(x.numpy(), None if add is None else add.numpy())
    e_model = np.abs(model.astype(np.float64) - ref.numpy()).max() / scale
    t32 = F.interpolate(x, scale_factor=2, mode="bicubic", align_corners=True)
    e_torch = ((t32 if add is None else add + t32).double() - ref).abs().max().item() / scale
    print("upsample %s add %s: float32 model %.3g, torch float32 CPU %.3g (of scale %.3g)"
          % (shape, with_add, e_model, e_torch, scale))
    assert model.dtype == np.float32 and e_model <= 1e-6
    assert e_torch <= 1e-6


def test_avgpool2_and_group_norm_are_torchs_float64_ops():
    for shape in ((2, 3, 2, 8), (1, 4, 6, 10), (3, 2, 10, 24)):
        x = er.values(shape, 5)
        got, want = er.avgpool2(x), F.avg_pool2d(x.double(), 2, stride=2)
        assert got.dtype == torch.float64 and got.shape == want.shape and (got - want).abs().max().item() <= 1e-15
    rows = (((2, 32, 2, 2), 32), ((2, 24, 6, 10), 1), ((2, 24, 6, 10), 3), ((3, 40, 2, 2), 40), ((1, 96, 3, 4), 32))
    for (n, c, h, w), groups in rows:
        x = er.values((n, c, h, w), 6) * 3 + 1.5
        res = er.noise((n, c, h, w), 7)
        g = torch.Generator().manual_seed(8)
        weight, bias, eps = torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5, 1e-5
        want = F.group_norm(x.double(), groups, weight.double(), bias.double(), eps)
        tol = 1e-12 * max(1.0, want.abs().max().item())
        assert (er.group_norm(x, groups, weight, bias, eps) - want).abs().max().item() <= tol
        assert (er.group_norm(x, groups, weight, bias, eps, relu=True) - torch.relu(want)).abs().max().item() <= tol
        with_res = er.group_norm(x, groups, weight, bias, eps, relu=True, res=res)
        assert (with_res - (torch.relu(want) + res.double())).abs().max().item() <= tol
        ss = er.scale_shift(x, groups, weight, bias, eps)
        assert ss.shape == (n, c, 2) and ss.dtype == torch.float64
        assert (x.double() * ss[..., 0, None, None] + ss[..., 1, None, None] - want).abs().max().item() <= tol


def test_upsample_route_agrees_with_the_lattice():
    """The admission rule of the banded kernel restated in Python against the route column, every class the GPU file's
    docstring names with at least one row, and the rule's edges one step either side."""
    for n, c, h, w, route, cls in er.UPSAMPLE_ROWS:
        assert er.upsample_route(c, h, w) == route and er.upsample_class(c, h, w) == cls, (n, c, h, w)
        assert (route == "banded") == (256 % (2 * w) == 0 and (2 * h) % 16 == 0 and (c // 32 * 2 * h) % 256 == 0)
    assert {r[5] for r in er.UPSAMPLE_ROWS} == set(er.UPSAMPLE_CLASSES)
    routes = [r[4] for r in er.UPSAMPLE_ROWS]
    assert routes.count("banded") == 6 and routes.count("element") == 9
    assert er.upsample_route(256, 64, 64) == "banded" and er.upsample_route(256, 128, 128) == "banded"  # the hourglass
    assert er.upsample_route(512, 8, 8) == "banded" and er.upsample_route(256, 8, 8) == "element"  # the slice rule
    assert er.upsample_route(32, 128, 128) == "banded" and er.upsample_route(32, 128, 130) == "element"


def test_library_predicate_is_the_restated_rule():
    """mp_upsample_gn_banded is host-only: the rule the launcher dispatches by against its Python restatement on the
    lattice and on a sweep of shapes around every clause."""
    from monoport_amd import _lib, build, ops
    build.build()
    lib = _lib.load()
    for n, c, h, w, route, _ in er.UPSAMPLE_ROWS:
        assert lib.mp_upsample_gn_banded(c, h, w) == (1 if route == "banded" else 0), (c, h, w)
    for c in (32, 64, 96, 160, 256, 512, 1024):
        for h in (2, 3, 4, 8, 12, 16, 24, 64, 128, 256):
            for w in (2, 4, 6, 8, 32, 64, 96, 128, 130, 256):
                assert ops.upsample_banded(c, h, w) == (er.upsample_route(c, h, w) == "banded"), (c, h, w)
    assert not ops.upsample_banded(48, 8, 8) and not ops.upsample_banded(0, 8, 8) and not ops.upsample_banded(32, 0, 8)
