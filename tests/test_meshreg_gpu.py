"""Mesh regularisers on the GPU (csrc/mesh_reg.hip, mesh_losses.py, OptimNetwork.computeTmpPcLoss) against the float64 restatement of
tests/_meshreg_ref.py.

Bounds (none of them comes from what the kernels give):
  values     every term is a sum of non-negative float32-representable terms of < 16 roundings each plus < 64 of an ordered block sum:
             |delta| <= 80 * 2^-24, relative for lap and edge, absolute for nc (a mean of terms in [0, 2]).
  gradients  two figures against float64 -- rms error over ALL vertices / rms of the gradient, largest per-vertex error / largest
             gradient -- and the same two for the FLOAT32 run of the restatement on the CPU; the kernels may have at most 4 x the
             restatement's figures (another summation order, other rounding in the normalisations).  No vertex is left out.
Every test prints its figures before it asserts; the operator-level ones also go to profiles/mesh_regularisers.json.

The kernels compute in double inside a thread and round once when they store, so their figures are expected at the float32 rounding of
the result (a numpy emulation of their algorithm gives 3e-8 to 1.2e-7 on the small meshes, where the float32 restatement has 2.6e-8 to
2.5e-6); the figures of a run are in profiles/mesh_regularisers.json."""
import json
import os

import numpy as np
import pytest
import torch

import _meshreg_ref as ref
from selfreconcode_amd.synthetic import icosphere

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_BOUND = 80. * 2. ** -24
TERMS = ("lap", "edge", "nc")
WEIGHTS = {"lap": (1., 0., 0.), "edge": (0., 1., 0.), "nc": (0., 0., 1.), "all": (1., 0.5, 0.25)}
FIGURES = {}


def bumpy_icosphere():
    v, f = icosphere(6)
    v = v.double()
    bump = 1. + 0.03 * torch.sin(9. * v[:, 0]) * torch.cos(7. * v[:, 1]) + 0.02 * torch.sin(13. * v[:, 2] + 1.)
    return (v * bump[:, None] * torch.tensor([1., 1.6, 0.7], dtype=torch.float64)).float(), f


def marching_cubes_template():
    from selfreconcode_amd.synthetic import build_synthetic_scene
    net, _, _ = build_synthetic_scene(device=DEV, frame_num=64, stage="coarse", consistent_masks=False)
    with torch.no_grad():
        v, f = net.discretizeSDF({'sdfRatio': 1., 'deformerRatio': 0.5, 'renderRatio': 1.}, None, 0.0)
    return v.detach().float().cpu(), f[(f >= 0).all(1)].long().cpu()


def small(name):
    v, f = ref.SMALL_MESHES[name]()
    return v.float(), f


MESHES = dict(icosphere6=bumpy_icosphere, strip=lambda: small("strip"), fan=lambda: small("fan"), unreferenced=lambda: small("unreferenced"),
              closed_small=lambda: icosphere(2), marching_cubes=marching_cubes_template)
_CACHE = {}


def mesh(name):
    """-> (verts float32 CPU, faces, loop-built topology, MeshTopology on the GPU); the float64 / float32 restatements per target length."""
    if name not in _CACHE:
        from selfreconcode_amd.mesh_losses import MeshTopology
        v, f = MESHES[name]()
        _CACHE[name] = dict(v=v, f=f, ref=ref.topology(f, v.shape[0]), topo=MeshTopology.from_faces(f.to(DEV), v.shape[0]), runs={})
    return _CACHE[name]


def restatement(m, target):
    if target not in m["runs"]:
        m["runs"][target] = (ref.values_and_grads(m["v"], m["ref"], target, torch.float64), ref.values_and_grads(m["v"], m["ref"], target, torch.float32))
    return m["runs"][target]


def run_op(m, weights, target, combine):
    from selfreconcode_amd.mesh_losses import mesh_regularisers
    v = m["v"].to(DEV).requires_grad_(True)
    out = mesh_regularisers(v, m["topo"], *weights, target_length=target)
    sum(w * o for w, o in zip(combine, out) if w != 0.).backward()
    return [float(o) for o in out], v.grad.double().cpu().numpy(), [o.detach().clone() for o in out], v.grad.clone()


@pytest.mark.parametrize("target", [0., 0.02])
@pytest.mark.parametrize("which", ["lap", "edge", "nc", "all"])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_values_and_gradients_against_float64(name, which, target):
    m = mesh(name)
    (val64, g64), (val32, g32) = restatement(m, target)
    w = WEIGHTS[which]
    vals, grad, _, _ = run_op(m, w, target, w)
    want = sum(wk * g for wk, g in zip(w, g64))
    theirs = ref.grad_errors(sum(wk * g for wk, g in zip(w, g32)), want)
    ours = ref.grad_errors(grad, want)
    dv = [abs(vals[k] - val64[k]) / (abs(val64[k]) if k < 2 and val64[k] != 0. else 1.) if w[k] > 0. else abs(vals[k]) for k in range(3)]
    fig = dict(V=int(m["v"].shape[0]), E=int(m["topo"].num_edges), P=int(m["topo"].num_pairs), value_error=dv, value_error_float32_restatement=[
        abs(val32[k] - val64[k]) / (abs(val64[k]) if k < 2 and val64[k] != 0. else 1.) for k in range(3)], kernel_rms=ours[0], kernel_max=ours[1],
        restatement_float32_rms=theirs[0], restatement_float32_max=theirs[1])
    FIGURES[f"{name}/{which}/t={target}"] = fig
    print(f"meshreg {name} {which} t={target}: {json.dumps(fig)}")
    for k in range(3):
        assert dv[k] <= VALUE_BOUND if w[k] > 0. else vals[k] == 0., (TERMS[k], vals[k], val64[k])
    assert ours[0] <= 4. * theirs[0] and ours[1] <= 4. * theirs[1], (ours, theirs)


def test_figures_are_recorded():
    """(runs after the parametrised test above in file order) -> profiles/mesh_regularisers.json"""
    assert FIGURES, "the value / gradient test did not run before this one"
    path = os.path.join(ROOT, "profiles", "mesh_regularisers.json")
    with open(path, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), value_bound=VALUE_BOUND, gradient_bound="4 x the float32 restatement's figure",
                       figures=FIGURES), fh, indent=1, sort_keys=True)
        fh.write("\n")


@pytest.mark.parametrize("name", ["icosphere6", "fan", "unreferenced"])
def test_two_runs_are_bit_equal(name):
    m = mesh(name)
    a, b = run_op(m, (1., 1., 1.), 0.02, (10., 10., 0.001)), run_op(m, (1., 1., 1.), 0.02, (10., 10., 0.001))
    for x, y in zip(a[2] + [a[3]], b[2] + [b[3]]):
        assert torch.equal(x, y)


def test_named_losses_and_unused_outputs():
    """pytorch3d's three names on the same op; an output that is not used costs no cotangent (the backward leaves its term out)."""
    from selfreconcode_amd import mesh_losses as ml
    m = mesh("closed_small")
    (val64, g64), _ = restatement(m, 0.)
    v = m["v"].to(DEV).requires_grad_(True)
    got = [ml.mesh_laplacian_smoothing(v, m["topo"]), ml.mesh_edge_loss(v, m["topo"]), ml.mesh_normal_consistency(v, m["topo"])]
    for k in range(3):
        assert abs(float(got[k]) - val64[k]) <= VALUE_BOUND * (abs(val64[k]) if k < 2 else 1.)
    lap, edge, nc = ml.mesh_regularisers(v, m["topo"], 1., 1., 1.)
    edge.backward()                                                                   # only the edge term is differentiated
    assert ref.grad_errors(v.grad.double().cpu().numpy(), g64[1])[1] < 16. * 2. ** -24        # (< 16 float32 roundings per vertex)
    t = float(ml.mesh_edge_loss(v, m["topo"], target_length=0.3))
    assert abs(t - float(ref.edge(m["v"].double(), m["ref"], 0.3))) <= VALUE_BOUND * t


# ------------------------------------------------------------------------------------------------ the step
RATIO = {'sdfRatio': 1., 'deformerRatio': 0.5, 'renderRatio': 1.}
STEP_WEIGHTS = (10., 10., 0.001)                                                      # the reference's magnitudes


def _scene():
    from selfreconcode_amd.synthetic import build_synthetic_scene
    net, ds, _ = build_synthetic_scene(device=DEV, frame_num=40, H=128, W=128, resolutions=[(15, 21, 9), (29, 41, 17), (57, 81, 33)],
                                       lbs_volume_shape=(17, 57, 33))
    net.conf['pc_weight']['def_consistent']['weight'] = -1.                           # (the call below passes no deformed template)
    return net, ds


def _set_weights(net, ws):
    for k, w in zip(('laplacian_weight', 'edge_weight', 'norm_weight'), ws):
        net.conf['pc_weight'][k] = w


def _template_call(net, V0):
    """computeTmpPcLoss from the saved template V0 with a mask that depends on the first 512 vertices; -> TmpVs.grad, info['pc_loss']"""
    net.TmpVs = V0.clone().requires_grad_(True)
    net.TmpOptimizer = torch.optim.SGD([net.TmpVs], lr=0.05, momentum=0.9)
    net.info['pc_loss'] = {}
    masks = torch.sigmoid(4. * net.TmpVs[:512, 0]).view(2, 16, 16)
    gt = (torch.arange(512, device=DEV) % 3 == 0).float().view(2, 16, 16)
    net.computeTmpPcLoss(None, None, masks, gt, RATIO)
    return net.TmpVs.grad.detach().double().cpu().numpy(), dict(net.info['pc_loss'])


def _check_step(net, V0, fresh=True):
    faces = net.Tmpfs[(net.Tmpfs >= 0).all(1)].cpu()
    t = ref.topology(faces, V0.shape[0])
    (val64, g64), (_, g32) = ref.values_and_grads(V0.float().cpu(), t, 0., torch.float64), ref.values_and_grads(V0.float().cpu(), t, 0., torch.float32)
    _set_weights(net, (-10., -10., -0.001))
    off, info_off = _template_call(net, V0)
    assert not {'lap_loss', 'edge_loss', 'norm_loss'} & set(info_off)
    if fresh:                                                                         # negative weights build no topology
        assert net._mesh_topo is None
    _set_weights(net, STEP_WEIGHTS)
    on, info = _template_call(net, V0)
    want = sum(w * g for w, g in zip(STEP_WEIGHTS, g64))
    theirs, ours = ref.grad_errors(sum(w * g for w, g in zip(STEP_WEIGHTS, g32)), want), ref.grad_errors(on - off, want)
    print(f"meshreg step V={V0.shape[0]}: kernel rms {ours[0]:.3e} max {ours[1]:.3e}; float32 restatement rms {theirs[0]:.3e} max {theirs[1]:.3e}; "
          f"values {[float(info[k]) for k in ('lap_loss', 'edge_loss', 'norm_loss')]} vs {val64}")
    for k, key in enumerate(('lap_loss', 'edge_loss', 'norm_loss')):
        assert info[key].is_cuda and not info[key].requires_grad
        assert abs(float(info[key]) - val64[k]) <= VALUE_BOUND * (abs(val64[k]) if k < 2 else 1.)
    assert net._mesh_topo[2].num_edges == t["edges"].shape[0] and net._mesh_topo[2].num_pairs == t["pairs"].shape[0]
    assert ours[0] <= 4. * theirs[0] and ours[1] <= 4. * theirs[1], (ours, theirs)


def test_step_adds_the_weighted_terms_and_follows_a_remesh():
    net, ds = _scene()
    net._remesh_if_due(RATIO, torch.device(DEV))
    _check_step(net, net.TmpVs.detach().clone())
    E0 = net._mesh_topo[2].num_edges
    net.forward_time, net.sdfShrinkRadius = 0, 0.03                                  # the next remesh extracts another level set
    net._remesh_if_due(RATIO, torch.device(DEV))
    assert net._mesh_topo is None, "a remesh must drop the cached topology"
    _check_step(net, net.TmpVs.detach().clone())
    assert net._mesh_topo[2].num_edges != E0
    # a caller that assigns Tmpfs directly (as the parity tests do) is caught by the key, not served the old topology
    keep = net.Tmpfs[: net.Tmpfs.shape[0] // 2].clone()
    stale, net.Tmpfs = net._mesh_topo[2], keep
    _check_step(net, net.TmpVs.detach().clone(), fresh=False)
    assert net._mesh_topo[2] is not stale


def test_full_iteration_with_positive_weights():
    """No positive-weight configuration stops the program any more: one whole iteration, finite, the three figures in info."""
    net, ds = _scene()
    _set_weights(net, STEP_WEIGHTS)
    fids = torch.tensor([3, 11, 20], device=DEV)
    loss = net(ds.batch(fids), 512, RATIO, fids)
    loss.backward()
    net.propagateTmpPsGrad(fids, RATIO)
    assert torch.isfinite(loss).item() and torch.isfinite(net.TmpVs).all().item()
    assert all(torch.isfinite(net.info['pc_loss'][k]).item() for k in ('lap_loss', 'edge_loss', 'norm_loss'))
