"""Mesh regularisers, the part that needs no GPU: the restated semantics reproduce the hand-checkable closed forms,
MeshTopology.from_faces (torch ops, here on CPU tensors) agrees with the independent loop-built topology of tests/_meshreg_ref.py,
and the operators refuse CPU tensors."""
import numpy as np
import pytest
import torch

import _meshreg_ref as ref
from selfreconcode_amd import mesh_losses
from selfreconcode_amd.mesh_losses import MeshTopology
from selfreconcode_amd.synthetic import icosphere


def test_closed_form_cube():
    v, f = ref.cube()
    t = ref.topology(f, 8)
    assert t["edges"].shape[0] == 18 and t["pairs"].shape[0] == 18
    assert abs(float(ref.edge(v, t)) - 4. / 3.) < 1e-12
    assert abs(float(ref.normal_consistency(v, t)) - 2. / 3.) < 1e-12


@pytest.mark.parametrize("a", [1., 0.37])
def test_closed_form_tetrahedron(a):
    v, f = ref.tetrahedron(a)
    t = ref.topology(f, 4)
    assert abs(float(ref.laplacian(v, t)) - a * 6. ** 0.5 / 3.) < 1e-12
    assert abs(float(ref.edge(v, t)) - a * a) < 1e-12
    assert abs(float(ref.edge(v, t, target_length=a))) < 1e-12
    assert abs(float(ref.normal_consistency(v, t)) - 4. / 3.) < 1e-12


def test_restatement_conventions():
    """|d_i| = 0 and zero-length edges contribute 0 with gradient 0; an unreferenced vertex has d_i = -v_i; no pair -> nc = 0."""
    v = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    t = ref.topology([[0, 1, 2]], 3)
    y = ref.laplacian(v, t) + ref.edge(v, t, 0.5) + ref.normal_consistency(v, t)
    g, = torch.autograd.grad(y, v)
    assert float(y.detach()) == 0.25 and torch.all(g == 0)
    v, f = ref.with_unreferenced()
    t = ref.topology(f, v.shape[0])
    assert t["deg"][4] == 0 and t["deg"][-1] == 0
    lone = torch.zeros_like(v); lone[4] = v[4]; lone[-1] = v[-1]
    only = ref.topology(torch.zeros((0, 3), dtype=torch.long), v.shape[0])
    assert abs(float(ref.laplacian(lone, only)) - float(v[4].norm() + v[-1].norm()) / v.shape[0]) < 1e-12


MESHES = dict(icosphere=lambda: icosphere(2), **ref.SMALL_MESHES)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_topology_matches_the_loop_built_one(name):
    v, f = MESHES[name]()
    V = v.shape[0]
    topo, t = MeshTopology.from_faces(f, V), ref.topology(f, V)
    for x in (topo.edges, topo.deg, topo.nbr_row, topo.nbr, topo.pairs, topo.pair_row, topo.pair_ent):
        assert x.dtype == torch.int32 and x.is_contiguous()
    assert np.array_equal(topo.edges.numpy(), t["edges"]) and np.array_equal(topo.deg.numpy(), t["deg"])
    assert topo.num_verts == V and topo.num_edges == len(t["edges"]) and topo.num_pairs == len(t["pairs"])
    row, nbr = topo.nbr_row.numpy(), topo.nbr.numpy()
    assert row[0] == 0 and row[-1] == 2 * topo.num_edges
    assert [nbr[row[i]:row[i + 1]].tolist() for i in range(V)] == t["nbrs"]
    assert np.array_equal(topo.pairs.numpy(), t["pairs"])
    prow, pent = topo.pair_row.numpy(), topo.pair_ent.numpy()
    flat = t["pairs"].reshape(-1)
    assert prow[0] == 0 and prow[-1] == flat.size
    for i in range(V):
        assert pent[prow[i]:prow[i + 1]].tolist() == np.nonzero(flat == i)[0].tolist()      # the vertex's (pair, slot) entries, ascending


def test_topology_counts():
    v, f = icosphere(2)
    topo = MeshTopology.from_faces(f, v.shape[0])
    assert topo.num_edges == 3 * f.shape[0] // 2 == topo.num_pairs                          # closed manifold: every edge has two faces
    v, f = ref.strip(6)
    topo = MeshTopology.from_faces(f, 12)
    assert topo.num_edges == 21 and topo.num_pairs == 9                                      # 12 boundary edges give no pair
    topo = MeshTopology.from_faces(ref.fan()[1], 5)
    assert topo.num_edges == 7 and topo.pairs.tolist() == [[0, 1, 2, 3], [0, 1, 2, 4], [0, 1, 3, 4]]
    topo = MeshTopology.from_faces(ref.with_unreferenced()[1], 12)
    assert topo.deg[4] == 0 and topo.deg[11] == 0 and topo.nbr_row[4] == topo.nbr_row[5]
    empty = MeshTopology.from_faces(torch.zeros((0, 3), dtype=torch.long), 4)
    assert empty.num_edges == 0 and empty.num_pairs == 0 and empty.nbr_row.tolist() == [0] * 5


def test_topology_rejects_bad_faces():
    with pytest.raises(ValueError):
        MeshTopology.from_faces(torch.tensor([[0, 1, 4]]), 4)
    with pytest.raises(ValueError):
        MeshTopology.from_faces(torch.tensor([[0, -1, 2]]), 4)
    with pytest.raises(ValueError):
        MeshTopology.from_faces(torch.tensor([[0., 1., 2.]]), 4)


def test_no_cpu_fallback():
    v, f = icosphere(1)
    topo = MeshTopology.from_faces(f, v.shape[0])
    with pytest.raises(RuntimeError):
        mesh_losses.mesh_regularisers(v, topo, 1., 1., 1.)
    for fn in (mesh_losses.mesh_laplacian_smoothing, mesh_losses.mesh_edge_loss, mesh_losses.mesh_normal_consistency):
        with pytest.raises(RuntimeError):
            fn(v, topo)
    from selfreconcode_amd import ops
    with pytest.raises(RuntimeError):
        ops.meshreg_fwd(v, topo.nbr_row, topo.nbr, topo.pairs, 7)
    with pytest.raises(RuntimeError):
        ops.meshreg_bwd((v, v, None), topo.nbr_row, topo.nbr, topo.pair_row, topo.pair_ent, v.shape[0], None, None, None)


@pytest.mark.parametrize("method", ["cot", "cotcurv"])
def test_only_the_uniform_laplacian_exists(method):
    v, f = icosphere(1)
    with pytest.raises(ValueError):
        mesh_losses.mesh_laplacian_smoothing(v, MeshTopology.from_faces(f, v.shape[0]), method=method)


def test_exported_and_configurable():
    import selfreconcode_amd
    for name in mesh_losses.__all__:
        assert getattr(selfreconcode_amd, name) is getattr(mesh_losses, name)
    from selfreconcode_amd.config import _loss, default_config
    pc = _loss(0.5, 2., 60., 10., 0.6, edge=10., norm=0.001)['pc_weight']
    assert (pc['laplacian_weight'], pc['edge_weight'], pc['norm_weight']) == (10., 10., 0.001)
    for stage in ("coarse", "medium", "fine"):                                                # shipped defaults: all three off
        pc = default_config().get_config('loss_' + stage)
        assert all(pc.get_float('pc_weight.' + k) < 0. for k in ('laplacian_weight', 'edge_weight', 'norm_weight'))
