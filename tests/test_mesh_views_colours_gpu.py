"""Multi-view netC colours in the mesh chain: recon.reconstruct_mesh / reconstruct_mesh_many(view=k) colour the vertices
through ViewsBindings and ops.query_views_counted_batch, on counts that never leave the device.  The reference is
netC.query (ops.query_views) on the mesh's own vertices, row k, as bits.  Needs an MI355X."""
import numpy as np
import pytest

from monoport_amd import synthetic as syn
from test_query_views_gpu import _net, calibs_of
from test_views_slot_gpu import same_mesh

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
BMIN, BMAX = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def ops():
    from monoport_amd import ops
    return ops


@pytest.fixture(scope="module", params=[2, 3])
def case(request):
    """A seeded multi-view netC of V views, two 33^3 volumes and per volume V random 16 x 16 x 512 maps and cameras; view
    1 of the first set is shifted partly off its image, so the rows of netC's result differ."""
    v_n = request.param
    net = _net("C", syn.rand_mlp("C", 810 + v_n, 2.0), v_n)
    vols = [torch.from_numpy(syn.sphere_volume(33)).to(DEV), torch.from_numpy(syn.sphere_volume(33, radius=0.45)).to(DEV)]
    feats = [[[torch.from_numpy(np.stack([syn.rand_feat(512, 16, 16, 820 + 10 * k + v) for v in range(v_n)])).to(DEV)]]
             for k in range(2)]
    calibs = [torch.from_numpy(calibs_of(dict(proj="orthogonal", steps=[50 * k + 23 * v for v in range(v_n)]))).to(DEV)
              for k in range(2)]
    calibs[0][1, 0, 3] += 0.7
    return dict(V=v_n, net=net, vols=vols, feats=feats, calibs=calibs)


def colours_of(net, feats, verts, calibs, k):
    """Row k of netC.query on the vertices, given to every view, as the mesh's colours."""
    v_n = calibs.shape[0]
    with torch.no_grad():
        pred = net.query(feats, verts.t()[None].expand(v_n, 3, verts.shape[0]), calibs)[0]
    return (pred[k] * 0.5 + 0.5).t()


def mesh_of(case, i, k, **kw):
    from monoport_amd.recon import reconstruct_mesh
    return reconstruct_mesh(case["vols"][i], 0.5, BMIN, BMAX, netC=case["net"], feat_tensor_C=case["feats"][i],
                            calib_tensor=case["calibs"][i], view=k, **kw)


def test_colours_are_row_k_of_the_query(ops, case):
    from monoport_amd.recon import reconstruct_mesh
    plain = reconstruct_mesh(case["vols"][0], 0.5, BMIN, BMAX)
    rows = []
    for k in range(case["V"]):
        mesh = mesh_of(case, 0, k)
        same_mesh(mesh._replace(colors=None), plain, "geometry, view %d" % k)
        want = colours_of(case["net"], case["feats"][0], mesh.verts, case["calibs"][0], k)
        assert mesh.verts.shape[0] > 1000 and mesh.colors.shape == mesh.verts.shape and mesh.colors.is_contiguous()
        assert torch.equal(mesh.colors, want), "view %d" % k
        rows.append(mesh.colors)
        # the colours of the simplified mesh are those of ITS vertices
        simple = mesh_of(case, 0, k, simplify=8)
        assert 0 < simple.verts.shape[0] < mesh.verts.shape[0] // 2
        assert torch.equal(simple.colors, colours_of(case["net"], case["feats"][0], simple.verts, case["calibs"][0], k))
        # smoothing moves the vertices, the colours are queried before it
        smooth = mesh_of(case, 0, k, smooth=2)
        assert not torch.equal(smooth.verts, mesh.verts) and torch.equal(smooth.faces, mesh.faces)
        assert torch.equal(smooth.colors.view(torch.int32), mesh.colors.view(torch.int32))
    # view 1's camera is partly off its image: exact 0 (colour 0.5) there, and the rows differ
    assert not torch.equal(rows[0], rows[1])
    off = (rows[1] == 0.5).all(1)
    assert 20 < int(off.sum()) < off.numel() - 20 and not (rows[0][off] == 0.5).all()


def test_many_equals_the_per_mesh_calls(ops, case):
    from monoport_amd.recon import reconstruct_mesh_many
    for k in range(case["V"]):
        many = reconstruct_mesh_many([case["vols"][0], None, case["vols"][1]], 0.5, BMIN, BMAX, netC=case["net"],
                                     feat_tensors_C=[case["feats"][0], None, case["feats"][1]],
                                     calib_tensors=[case["calibs"][0], None, case["calibs"][1]], view=k, simplify=12)
        assert many[1] is None
        same_mesh(many[0], mesh_of(case, 0, k, simplify=12), "volume 0, view %d" % k)
        same_mesh(many[2], mesh_of(case, 1, k, simplify=12), "volume 2, view %d" % k)
        assert not torch.equal(many[0].verts, many[2].verts)


def test_short_capacity_rerun_keeps_the_colours(ops, case, monkeypatch):
    """Marching cubes' capacity guess cut short: the chain runs again through _mesh_chains(max_verts=...), with the same
    multi-view colour query."""
    k = case["V"] - 1
    mesh = mesh_of(case, 0, k)
    real, calls = ops.marching_cubes_raw_batch, []

    def short(volumes, level=0.5, b_min=(-1, -1, -1), b_max=(1, 1, 1), max_verts=None, max_faces=None, **kw):
        calls.append((max_verts, max_faces))
        if max_verts is None:
            max_verts, max_faces = 300, 500
        return real(volumes, level, b_min, b_max, max_verts=max_verts, max_faces=max_faces, **kw)

    monkeypatch.setattr(ops, "marching_cubes_raw_batch", short)
    again = mesh_of(case, 0, k)
    monkeypatch.undo()
    assert calls == [(None, None), (mesh.verts.shape[0], mesh.faces.shape[0])]
    same_mesh(again, mesh, "re-run")


def test_dirty_arena_gives_the_same_bits(ops, case):
    k = 0
    mesh = mesh_of(case, 0, k, simplify=8)
    assert ops.scratch_fill(DEV, 64 << 20, 0xFF) >= 64 << 20
    same_mesh(mesh_of(case, 0, k, simplify=8), mesh, "on 0xFF residue")
