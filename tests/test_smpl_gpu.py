"""The SMPL body model on the GPU (csrc/smpl.hip behind smpl_pytorch.SMPL) against the float64 twin of tests/_smpl_ref.py and, at
nv = 200, against what the reference's own class gave (tests/golden/smpl.npz).

Bound, per output: BOUND_FACTOR (4) times the float32-against-float64 error the golden generator recorded for the reference's own
evaluation of that output -- the same sums taken in another order over 207 and nv terms.  v_shaped has no recorded error of its own:
it is an intermediate of `verts` with 11 of its terms, so the bound of `verts` covers it.

Measured on an MI355X, largest |product - twin| over every case below (bound): verts 4.7e-7 (1.8e-6), joints 3.0e-7 (7.7e-7),
Rs 2.2e-7 (7.7e-7), J 6.3e-7 (2.6e-6), J_transformed 5.8e-7 (1.9e-6), A 7.3e-7 (3.2e-6), avatar 7.1e-7 (1.6e-6), v_shaped 6.8e-8;
the table is in profiles/smpl_body.md.
"""
import functools
import os

import numpy as np
import pytest
import torch

import _smpl_ref as twin
from selfreconcode_amd import ops
from selfreconcode_amd.synthetic import det_array, synthetic_smpl_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = ops.SMPL_BATCH_TILE
NVS = (200, 1500, 63)            # the golden case, not a multiple of 64 / several workgroups and chunks of the reductions / less than one wave
BATCHES = (1, TILE, TILE + 1)


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "smpl.npz")))


def _bound(name):
    return twin.BOUND_FACTOR * float(_gold()["err_" + {"v_shaped": "verts", "joints_lsp": "joints_lsp"}.get(name, name)])


@functools.lru_cache(maxsize=None)
def _model(nv):
    return synthetic_smpl_model(nv, twin.GOLDEN_SEED)


@functools.lru_cache(maxsize=None)
def _smpl(nv, joint_type='cocoplus'):
    from selfreconcode_amd.smpl_pytorch import SMPL
    return SMPL(_model(nv), joint_type=joint_type, obj_saveable=True).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(nv, B):
    """(beta, theta, float64 twin outputs) -- computed once, shared, never written to."""
    beta, theta = twin.golden_inputs(B, seed=0 if B == twin.GOLDEN_B else B)
    return beta, theta, twin.forward(_model(nv), beta, theta, Tvs=_model(nv)["v_template"])


def _check(name, got, want, what=""):
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    e = float(np.abs(got - want).max())
    print(f"{what} {name}: error {e:.3e}, bound {_bound(name):.3e}")
    assert np.isfinite(got).all() and e <= _bound(name), (what, name, e, _bound(name))


def _run(smpl, beta, theta):
    verts, joints, Rs = smpl(torch.from_numpy(beta).to(DEV), torch.from_numpy(theta).to(DEV), get_skin=True)
    return {"verts": verts, "joints": joints, "Rs": Rs, "J": smpl.J, "J_transformed": smpl.J_transformed, "A": smpl.A}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("nv", NVS)
def test_forward_matches_the_float64_twin(nv, B):
    beta, theta, want = _case(nv, B)
    got = _run(_smpl(nv), beta, theta)
    assert got["verts"].shape == (B, nv, 3) and got["joints"].shape == (B, 19, 3) and got["A"].shape == (B, 24, 4, 4)
    for name, value in got.items():
        _check(name, value, want[name], f"nv={nv} B={B}")
    again = _run(_smpl(nv), beta, theta)
    assert all(torch.equal(again[k], got[k]) for k in got)                  # no atomics: bit for bit


def test_golden_case_matches_the_reference_and_the_twin():
    gold = _gold()
    nv = twin.GOLDEN_NV
    assert twin.model_sha256(_model(nv)) == str(gold["model_sha256"])
    beta, theta, want = _case(nv, twin.GOLDEN_B)
    smpl = _smpl(nv)
    got = _run(smpl, beta, theta)
    got["avatar"] = smpl.avatar(torch.from_numpy(_model(nv)["v_template"]).to(DEV), torch.from_numpy(beta).to(DEV), torch.from_numpy(theta).to(DEV))
    for name in twin.OUTPUTS:
        _check(name, got[name], want[name], "golden case, twin")
        _check(name, got[name], gold[name].astype(np.float64), "golden case, reference")
    lsp = _smpl(nv, 'lsp')(torch.from_numpy(beta).to(DEV), torch.from_numpy(theta).to(DEV))
    assert lsp.shape == (twin.GOLDEN_B, 14, 3)
    _check("joints_lsp", lsp, gold["joints_lsp"].astype(np.float64), "golden case, reference")
    _check("joints_lsp", lsp, want["joints"][:, :14], "golden case, twin")
    assert torch.equal(lsp, got["joints"][:, :14])                            # the same sums over the first 14 columns


@pytest.mark.parametrize("nv,B", [(200, TILE + 1), (1500, 1), (63, TILE)])
def test_zero_pose_is_the_identity_and_leaves_the_shaped_body(nv, B):
    beta = twin.golden_inputs(B, seed=40)[0]
    theta = np.zeros((B, 24, 3), np.float32)
    smpl = _smpl(nv)
    got = _run(smpl, beta, theta)
    eye = torch.eye(3, device=DEV).expand(B, 24, 3, 3)
    assert float((got["Rs"] - eye).abs().max()) <= 1e-6                       # through the 1e-8 route
    want = twin.forward(_model(nv), beta, theta)
    for name, value in got.items():
        _check(name, value, want[name], f"theta=0 nv={nv} B={B}")
    J, v_shaped = smpl.skeleton(torch.from_numpy(beta).to(DEV), True)
    _check("v_shaped", v_shaped, want["v_shaped"], "theta=0")
    _check("verts", got["verts"], v_shaped.double().cpu().numpy(), "theta=0, verts against the shaped body")
    assert torch.equal(J, got["J"])


def test_a_joint_turned_by_nearly_pi():
    nv, B = 200, 2
    beta = twin.golden_inputs(B, seed=41)[0]
    theta = np.zeros((B, 24, 3), np.float32)
    theta[0, 0] = [3.14159, 0., 0.]
    theta[1, 18] = np.array([1., -1., 1.], np.float32) * np.float32(3.1415 / np.sqrt(3.))
    want = twin.forward(_model(nv), beta, theta)
    assert np.abs(np.trace(want["Rs"][0, 0]) + 1.) < 1e-4                     # a half turn
    for name, value in _run(_smpl(nv), beta, theta).items():
        _check(name, value, want[name], "nearly pi")


@pytest.mark.parametrize("nv,B", [(200, TILE), (63, 1)])
def test_rotation_matrices_as_input(nv, B):
    beta, theta, want = _case(nv, B)
    Rs64 = twin.rodrigues(theta.reshape(-1, 3)).reshape(B, 24, 3, 3)
    Rs32 = Rs64.astype(np.float32)
    want = twin.forward(_model(nv), beta, Rs32, theta_in_rodrigues=False)
    smpl = _smpl(nv)
    verts, joints, Rs = smpl(torch.from_numpy(beta).to(DEV), torch.from_numpy(Rs32).to(DEV), get_skin=True, theta_in_rodrigues=False)
    assert torch.equal(Rs.cpu(), torch.from_numpy(Rs32))
    for name, value in (("verts", verts), ("joints", joints), ("J_transformed", smpl.J_transformed), ("A", smpl.A)):
        _check(name, value, want[name], f"matrices nv={nv} B={B}")
    flat = smpl(torch.from_numpy(beta).to(DEV), torch.from_numpy(Rs32.reshape(B, 24 * 9)).to(DEV), theta_in_rodrigues=False)
    assert torch.equal(flat, joints)


@pytest.mark.parametrize("nv,B", [(200, TILE + 1), (1500, TILE)])
def test_lsp_joints_skeleton_and_joints_only(nv, B):
    beta, theta, want = _case(nv, B)
    tb, tt = torch.from_numpy(beta).to(DEV), torch.from_numpy(theta).to(DEV)
    lsp = _smpl(nv, 'lsp')
    joints = lsp(tb, tt)                                                       # get_skin=False: the joints alone
    assert torch.is_tensor(joints) and joints.shape == (B, 14, 3)
    _check("joints_lsp", joints, want["joints"][:, :14], f"lsp nv={nv} B={B}")
    full = _smpl(nv)
    only = full(tb, tt, get_skin=False)
    assert torch.equal(only, full(tb, tt, get_skin=True)[1]) and torch.equal(only[:, :14], joints)
    J, v_shaped = full.skeleton(tb, require_body=True)
    _check("J", J, want["J"], "skeleton"); _check("v_shaped", v_shaped, want["v_shaped"], "skeleton")
    assert torch.equal(full.skeleton(tb), J) and torch.equal(J, full.J)


@pytest.mark.parametrize("nv,B", [(200, 1), (1500, TILE + 1), (63, TILE)])
def test_avatar_skins_the_callers_vertices(nv, B):
    beta, theta, want = _case(nv, B)
    smpl = _smpl(nv)
    tv = torch.from_numpy(_model(nv)["v_template"]).to(DEV)
    out = smpl.avatar(tv, torch.from_numpy(beta).to(DEV), torch.from_numpy(theta).to(DEV))
    _check("avatar", out, want["avatar"], f"avatar nv={nv} B={B}")
    _check("J_transformed", smpl.J_transformed, want["J_transformed"], "avatar")
    other = det_array((nv, 3), 733, 0.5)
    w2 = twin.skin(_model(nv), np.broadcast_to(other.astype(np.float64)[None], (B, nv, 3)), want["A"])
    _check("avatar", smpl.avatar(torch.from_numpy(other).to(DEV), torch.from_numpy(beta).to(DEV), torch.from_numpy(theta).to(DEV)), w2, "avatar, other mesh")


def test_non_contiguous_and_double_inputs():
    nv, B = 200, TILE + 1
    beta, theta, want = _case(nv, B)
    smpl = _smpl(nv)
    ref = _run(smpl, beta, theta)
    wide = torch.zeros((B, 20), device=DEV)
    wide[:, ::2] = torch.from_numpy(beta).to(DEV)
    nc_beta = wide[:, ::2]
    nc_theta = torch.from_numpy(np.ascontiguousarray(theta.transpose(1, 0, 2))).to(DEV).transpose(0, 1)
    assert not nc_beta.is_contiguous() and not nc_theta.is_contiguous()
    verts, joints, Rs = smpl(nc_beta, nc_theta, get_skin=True)
    assert torch.equal(verts, ref["verts"]) and torch.equal(joints, ref["joints"]) and torch.equal(Rs, ref["Rs"])
    verts64 = smpl(nc_beta.double(), nc_theta.double().reshape(B, 72), get_skin=True)[0]
    assert torch.equal(verts64, ref["verts"])


def test_grad_and_cpu_inputs_raise():
    smpl = _smpl(200)
    beta, theta = torch.zeros((1, 10), device=DEV), torch.zeros((1, 24, 3), device=DEV)
    for args in ((beta.clone().requires_grad_(True), theta), (beta, theta.clone().requires_grad_(True))):
        with pytest.raises(NotImplementedError, match="forward only"):
            smpl(*args)
    with pytest.raises(NotImplementedError, match="forward only"):
        smpl.skeleton(beta.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError, match="forward only"):
        smpl.avatar(smpl.v_template.clone().requires_grad_(True), beta, theta)
    with torch.no_grad():                                                      # nothing to differentiate: allowed
        smpl(beta.clone().requires_grad_(True), theta)
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        smpl(beta.cpu(), theta)
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        smpl(beta, theta.cpu())
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        smpl.avatar(smpl.v_template.cpu(), beta, theta)


def test_kernel_argument_checks():
    from selfreconcode_amd import _lib
    smpl = _smpl(200)
    J = torch.zeros((1, 24, 3), device=DEV)
    bad = list(smpl.parents); bad[5] = 7                                       # a parent after its child
    with pytest.raises(_lib.SrError):
        ops.smpl_pose(J, bad, theta=torch.zeros((1, 24, 3), device=DEV))
    with pytest.raises(ValueError):
        ops.smpl_pose(J, smpl.parents)
    with pytest.raises(ValueError):
        ops.smpl_skin(torch.zeros((1, 199, 3), device=DEV), smpl.weight[0], torch.zeros((1, 24, 4, 4), device=DEV))
