"""The differentiable body model on the GPU (csrc/smpl_grad.hip behind smpl_pytorch.DifferentiableSMPL and the ops wrappers) against
the float64 twin of tests/_smplgrad_ref.py (gradients by torch autograd on CPU operators) and, at nv = 200, against the reference's
own float64 gradients (tests/golden/smpl_grad.npz).

Bounds.  g_beta, g_theta, gA, gJ and the avatar's three gradients: BOUND_FACTOR (4) times the float32-against-float64 error the
golden generator recorded for the reference's own evaluation of that gradient; the cotangents are scaled by sqrt(200 / nv) so that
the sums over the vertices keep the size they have in the golden case.  g_rest and g_feature are intermediates the reference's class
does not expose, so no error is recorded for them; their bound is the a-priori rounding bound of the sums they are,
(n + 8) u S with u = 2^-24, S the largest sum of the terms' absolute values (float64, from the twin) and n the number of roundings one
term passes through: 72 for g_rest = (sum_j w_j R_j)^T gV (serial sums); for g_feature the depth of its fixed tree -- 3 products per
lane, 6 butterfly levels over the wave, the 2 waves, ceil(nv / 128) partial rows -- plus the 80 of the g_rest it is formed from.  The 8
covers the float32 rounding of the inputs themselves.

Measured on an MI355X, largest |product - twin| over every case below (bound): g_beta 1.9e-7 (1.4e-6), g_theta 3.3e-6 (9.2e-6),
gA 6.9e-7 (2.8e-6), gJ 2.6e-6 (1.3e-5), avatar g_Tvs 2.4e-6 (5.7e-6), avatar g_beta 1.1e-7 (4.5e-7), avatar g_theta 4.5e-6 (5.0e-6),
g_rest 7.6e-8 (2.8e-6), g_feature 5.0e-8 (4.3e-5, nv = 1500; 2.8e-8 against 8.6e-6 at nv = 63); no factor above 4 was needed.  The table is in profiles/smpl_fit.md.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _smpl_ref as twin
import _smplgrad_ref as gtwin
from selfreconcode_amd import ops
from selfreconcode_amd.synthetic import det_array, synthetic_smpl_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
TILE = ops.SMPL_BATCH_TILE
NVS = (63, 200, 1500)            # less than a wave / the golden size / several workgroups and partial rows
BATCHES = (1, TILE, TILE + 1)    # ... and one item past a batch tile
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "smpl_grad.npz")))


def _bound(name):
    return gtwin.BOUND_FACTOR * float(_gold()["err_" + name])


@functools.lru_cache(maxsize=None)
def _model(nv):
    return synthetic_smpl_model(nv, twin.GOLDEN_SEED)


@functools.lru_cache(maxsize=None)
def _smpl(nv, joint_type='cocoplus', plain=False):
    from selfreconcode_amd.smpl_pytorch import SMPL, DifferentiableSMPL
    return (SMPL if plain else DifferentiableSMPL)(_model(nv), joint_type=joint_type, obj_saveable=True).to(DEV)


def _cots(B, nv, nk=19):
    from gen_smpl_grad_golden import cotangents
    return cotangents(B, nv, nk)


@functools.lru_cache(maxsize=None)
def _case(nv, B):
    """(beta, theta, Cv, Cj, the twin's float64 gradients and cotangents) -- computed once, shared, never written to."""
    beta, theta = twin.golden_inputs(B, seed=0 if B == twin.GOLDEN_B else B)
    Cv, Cj = _cots(B, nv)
    return beta, theta, Cv, Cj, gtwin.gradients(_model(nv), beta, theta, Cv, Cj)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(DEV)


def _check(name, got, want, bound, what=""):
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    e = float(np.abs(got - want).max())
    print(f"{what} {name}: error {e:.3e}, bound {bound:.3e}")
    assert np.isfinite(got).all() and e <= bound, (what, name, e, bound)


def _grads(smpl, beta, theta, Cv, Cj, Cr=None, in_rodrigues=True):
    tb, tt = _dev(beta).requires_grad_(True), _dev(theta).requires_grad_(True)
    verts, joints, Rs = smpl(tb, tt, get_skin=True, theta_in_rodrigues=in_rodrigues)
    L = (_dev(Cv) * verts).sum() + (_dev(Cj) * joints).sum()
    if Cr is not None:
        L = L + (_dev(Cr) * Rs).sum()
    return torch.autograd.grad(L, [tb, tt])


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("nv", NVS)
def test_forward_gradients_match_the_float64_twin(nv, B):
    beta, theta, Cv, Cj, want = _case(nv, B)
    g_beta, g_theta = _grads(_smpl(nv), beta, theta, Cv, Cj)
    _check("g_beta", g_beta, want["g_beta"], _bound("g_beta"), f"nv={nv} B={B}")
    _check("g_theta", g_theta, want["g_theta"], _bound("g_theta"), f"nv={nv} B={B}")
    again = _grads(_smpl(nv), beta, theta, Cv, Cj)
    assert torch.equal(again[0], g_beta) and torch.equal(again[1], g_theta)      # no atomics, fixed orders: bit for bit


def test_golden_case_matches_the_reference():
    gold = _gold()
    nv, B = twin.GOLDEN_NV, twin.GOLDEN_B
    assert twin.model_sha256(_model(nv)) == str(gold["model_sha256"])
    beta, theta, Cv, Cj, _ = _case(nv, B)
    g_beta, g_theta = _grads(_smpl(nv), beta, theta, Cv, Cj)
    _check("g_beta", g_beta, gold["g_beta"], _bound("g_beta"), "golden")
    _check("g_theta", g_theta, gold["g_theta"], _bound("g_theta"), "golden")
    tv, tb, tt = (_dev(x).requires_grad_(True) for x in (_model(nv)["v_template"], beta, theta))
    g = torch.autograd.grad((_dev(Cv) * _smpl(nv).avatar(tv, tb, tt)).sum(), [tv, tb, tt])
    for name, got in zip(("avatar_g_Tvs", "avatar_g_beta", "avatar_g_theta"), g):
        _check(name, got, gold[name], _bound(name), "golden")


@pytest.mark.parametrize("nv,B", [(63, TILE + 1), (200, 1), (1500, TILE)])
def test_avatar_gradients_reach_Tvs_beta_and_theta(nv, B):
    beta, theta, Cv, _, _ = _case(nv, B)
    Tvs = det_array((nv, 3), 733, 0.5)
    want = gtwin.avatar_gradients(_model(nv), Tvs, beta, theta, Cv)
    smpl = _smpl(nv)
    tv, tb, tt = (_dev(x).requires_grad_(True) for x in (Tvs, beta, theta))
    out = smpl.avatar(tv, tb, tt)
    assert not smpl.J_transformed.requires_grad
    g = torch.autograd.grad((_dev(Cv) * out).sum(), [tv, tb, tt])
    _check("avatar_g_Tvs", g[0], want["g_Tvs"], _bound("avatar_g_Tvs"), f"nv={nv} B={B}")
    _check("avatar_g_beta", g[1], want["g_beta"], _bound("avatar_g_beta"), f"nv={nv} B={B}")
    _check("avatar_g_theta", g[2], want["g_theta"], _bound("avatar_g_theta"), f"nv={nv} B={B}")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("nv", NVS)
def test_each_kernel_against_the_twins_cotangents(nv, B):
    beta, theta, Cv, Cj, want = _case(nv, B)
    model = _model(nv)
    m = gtwin.Model(model)
    fwd = {k: v.detach().numpy() for k, v in gtwin.forward(m, beta.astype(np.float64), theta.astype(np.float64)).items()}
    smpl = _smpl(nv)
    what = f"nv={nv} B={B}"
    # the joints' cotangent onto the vertices, added to the vertices' own
    gV = ops.smpl_regress_bwd(_dev(Cj), smpl.joint_regressor, out=_dev(Cv))
    S = np.abs(Cv).astype(np.float64) + np.einsum('vk,bkc->bvc', np.abs(model['cocoplus_regressor']).astype(np.float64), np.abs(Cj))
    _check("gV", gV, want["gV"], (19 + 8) * U * float(S.max()), what)
    # the skin stage
    A32, feat32, vs32 = _dev(fwd["A"]), _dev(fwd["feature"]), _dev(fwd["v_shaped"])
    g_rest, gA, g_feature = ops.smpl_skin_bwd(vs32, smpl.weight[0], A32, _dev(want["gV"]), smpl.posedirs, feat32)
    absT = np.einsum('vj,bjrc->bvrc', model['weights'].astype(np.float64), np.abs(fwd["A"][:, :, :3, :3]))
    S_rest = np.einsum('bvrc,bvr->bvc', absT, np.abs(want["gV"]))
    _check("g_rest", g_rest, want["g_rest"], (72 + 8) * U * float(S_rest.max()), what)
    S_feat = np.einsum('vck,bvc->bk', np.abs(model['posedirs']).astype(np.float64), S_rest)
    depth = 3 + 6 + 1 + -(-nv // 128)            # 3 products per lane, 6 butterfly levels, 2 waves, the partial rows of 128 vertices
    _check("g_feature", g_feature, want["g_feature"], (depth + 80 + 8) * U * float(S_feat.max()), what)
    _check("gA", gA, want["gA"], _bound("gA"), what)
    # the pose stage
    g_theta, gJ = ops.smpl_pose_bwd(_dev(fwd["Rs"]), _dev(fwd["J"]), A32, smpl.parents, theta=_dev(theta), gA=_dev(want["gA"]),
                                    g_feature=_dev(want["g_feature"]))
    _check("g_theta", g_theta, want["g_theta"], _bound("g_theta"), what)
    _check("gJ", gJ, want["gJ"], _bound("gJ"), what)
    # the rest joints' cotangent onto v_shaped, then the shape stage
    g_vs = ops.smpl_regress_bwd(_dev(want["gJ"]), smpl.J_regressor, out=_dev(want["g_rest"]))
    g_beta = ops.smpl_shape_bwd(smpl.shapedirs, g_vs)
    _check("g_beta", g_beta, want["g_beta"], _bound("g_beta"), what)
    fresh = ops.smpl_regress_bwd(_dev(want["gJ"]), smpl.J_regressor)
    assert torch.equal(fresh + _dev(want["g_rest"]), g_vs)                      # accumulate = the same sum, added once


@pytest.mark.parametrize("nv,B", [(200, TILE + 1), (63, 1)])
def test_zero_pose_takes_the_1e8_route(nv, B):
    beta = twin.golden_inputs(B, seed=40)[0]
    theta = np.zeros((B, 24, 3), np.float32)
    Cv, Cj = _cots(B, nv)
    want = gtwin.gradients(_model(nv), beta, theta, Cv, Cj)
    assert np.isfinite(want["g_theta"]).all()
    g_beta, g_theta = _grads(_smpl(nv), beta, theta, Cv, Cj)
    _check("g_beta", g_beta, want["g_beta"], _bound("g_beta"), "theta=0")
    _check("g_theta", g_theta, want["g_theta"], _bound("g_theta"), "theta=0")


def test_a_joint_turned_by_nearly_pi():
    nv, B = 200, 2
    beta = twin.golden_inputs(B, seed=41)[0]
    theta = np.zeros((B, 24, 3), np.float32)
    theta[0, 0] = [3.14159, 0., 0.]
    theta[1, 18] = np.array([1., -1., 1.], np.float32) * np.float32(3.1415 / np.sqrt(3.))
    Cv, Cj = _cots(B, nv)
    want = gtwin.gradients(_model(nv), beta, theta, Cv, Cj)
    g_beta, g_theta = _grads(_smpl(nv), beta, theta, Cv, Cj)
    _check("g_beta", g_beta, want["g_beta"], _bound("g_beta"), "nearly pi")
    _check("g_theta", g_theta, want["g_theta"], _bound("g_theta"), "nearly pi")


@pytest.mark.parametrize("nv,B", [(200, TILE), (63, 1)])
def test_rotation_matrices_as_input_and_a_cotangent_on_Rs(nv, B):
    beta, theta, Cv, Cj, _ = _case(nv, B)
    Rs32 = twin.rodrigues(theta.reshape(-1, 3)).reshape(B, 24, 3, 3).astype(np.float32)
    Cr = det_array((B, 24, 3, 3), 742, 1.0)
    want = gtwin.gradients(_model(nv), beta, Rs32, Cv, Cj, Cr, theta_in_rodrigues=False)
    g_beta, g_R = _grads(_smpl(nv), beta, Rs32, Cv, Cj, Cr, in_rodrigues=False)
    assert g_R.shape == (B, 24, 3, 3)
    _check("g_beta", g_beta, want["g_beta"], _bound("g_beta"), "matrices")
    _check("g_theta", g_R, want["g_theta"], _bound("g_theta"), "matrices (the gradient of the rotations)")
    # axis-angle input with a cotangent on Rs alone: only the pose kernel runs
    want = gtwin.gradients(_model(nv), beta, theta, None, None, Cr)
    tb, tt = _dev(beta).requires_grad_(True), _dev(theta).requires_grad_(True)
    Rs = _smpl(nv)(tb, tt, get_skin=True)[2]
    g_theta = torch.autograd.grad((_dev(Cr) * Rs).sum(), tt)[0]
    _check("g_theta", g_theta, want["g_theta"], _bound("g_theta"), "cotangent on Rs")


@pytest.mark.parametrize("nv,B", [(200, TILE + 1), (1500, 1)])
def test_lsp_joints_and_the_joints_only_path(nv, B):
    beta, theta, _, _, _ = _case(nv, B)
    for joint_type, nk in (("lsp", 14), ("cocoplus", 19)):
        Cj = _cots(B, nv, nk)[1]
        want = gtwin.gradients(_model(nv), beta, theta, None, Cj, joint_type=joint_type)
        tb, tt = _dev(beta).requires_grad_(True), _dev(theta).requires_grad_(True)
        smpl = _smpl(nv, joint_type)
        joints = smpl(tb, tt)                                                   # get_skin=False
        assert torch.is_tensor(joints) and joints.shape == (B, nk, 3) and joints.requires_grad
        assert not smpl.J.requires_grad and not smpl.A.requires_grad and not smpl.J_transformed.requires_grad
        g_beta, g_theta = torch.autograd.grad((_dev(Cj) * joints).sum(), [tb, tt])
        _check("g_beta", g_beta, want["g_beta"], _bound("g_beta"), f"{joint_type} joints only")
        _check("g_theta", g_theta, want["g_theta"], _bound("g_theta"), f"{joint_type} joints only")


def test_skeleton_is_differentiable_in_beta():
    nv, B = 200, TILE + 1
    beta = twin.golden_inputs(B, seed=B)[0]
    CJ, Cvs = det_array((B, 24, 3), 743, 1.0), det_array((B, nv, 3), 744, 1.0)
    m = gtwin.Model(_model(nv))
    b64 = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    v_shaped = m.v_template.unsqueeze(0) + torch.einsum('vck,bk->bvc', m.shapedirs, b64)
    J = torch.einsum('vj,bvc->bjc', m.J_regressor, v_shaped)
    want = torch.autograd.grad((torch.from_numpy(CJ.astype(np.float64)) * J).sum() + (torch.from_numpy(Cvs.astype(np.float64)) * v_shaped).sum(), b64)[0].numpy()
    tb = _dev(beta).requires_grad_(True)
    J_gpu, vs_gpu = _smpl(nv).skeleton(tb, require_body=True)
    got = torch.autograd.grad((_dev(CJ) * J_gpu).sum() + (_dev(Cvs) * vs_gpu).sum(), tb)[0]
    _check("g_beta", got, want, _bound("g_beta"), "skeleton")
    got_J = torch.autograd.grad((_dev(CJ) * _smpl(nv).skeleton(tb)).sum(), tb)[0]
    assert torch.isfinite(got_J).all() and got_J.shape == (B, 10)


def test_without_grad_it_is_the_plain_model_bit_for_bit():
    nv, B = 200, TILE + 1
    beta, theta, _, _, _ = _case(nv, B)
    plain, diff = _smpl(nv, plain=True), _smpl(nv)
    tb, tt, tv = _dev(beta), _dev(theta), _dev(_model(nv)["v_template"])
    want = plain(tb, tt, get_skin=True)
    for got in (diff(tb, tt, get_skin=True),                                               # nothing requires grad
                diff(tb.clone().requires_grad_(True), tt.clone().requires_grad_(True), get_skin=True)):      # the Function's own forward
        assert all(torch.equal(a.detach(), b) for a, b in zip(got, want))
    assert torch.equal(diff.J, plain.J) and torch.equal(diff.A, plain.A) and torch.equal(diff.J_transformed, plain.J_transformed)
    with torch.no_grad():
        got = diff(tb.clone().requires_grad_(True), tt, get_skin=True)
    assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(got, want))
    assert torch.equal(diff.avatar(tv, tb, tt), plain.avatar(tv, tb, tt))
    assert torch.equal(diff.avatar(tv.clone().requires_grad_(True), tb, tt).detach(), plain.avatar(tv, tb, tt))
    assert torch.equal(diff.skeleton(tb), plain.skeleton(tb))
    assert torch.equal(diff.skeleton(tb.clone().requires_grad_(True)).detach(), plain.skeleton(tb))


def test_double_backward_raises_and_the_plain_model_still_refuses():
    nv = 200
    beta, theta = torch.zeros((1, 10), device=DEV), torch.zeros((1, 24, 3), device=DEV)
    tb = beta.clone().requires_grad_(True)
    joints = _smpl(nv)(tb, theta)
    with pytest.raises(NotImplementedError, match="again"):
        torch.autograd.grad(joints.sum(), tb, create_graph=True)
    with pytest.raises(NotImplementedError, match="forward only"):
        _smpl(nv, plain=True)(tb, theta)
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        _smpl(nv)(tb.detach().cpu().requires_grad_(True), theta)


def test_kernel_argument_checks():
    from selfreconcode_amd import _lib
    smpl = _smpl(200)
    z = lambda *s: torch.zeros(s, device=DEV)          # noqa: E731
    bad = list(smpl.parents); bad[5] = 7
    with pytest.raises(_lib.SrError):
        ops.smpl_pose_bwd(z(1, 24, 3, 3), z(1, 24, 3), z(1, 24, 4, 4), bad, theta=z(1, 24, 3))
    with pytest.raises(ValueError):
        ops.smpl_skin_bwd(z(1, 200, 3), smpl.weight[0], z(1, 24, 4, 4), z(1, 199, 3))
    with pytest.raises(ValueError):
        ops.smpl_regress_bwd(z(1, 19, 3), smpl.J_regressor)
    with pytest.raises(_lib.SrError):
        ops.keypoint_energy(z(1, 65, 3), z(1, 3), z(1, 65, 3), z(65), [0.] * 16, 100.)
    with pytest.raises(_lib.SrError):
        ops.keypoint_energy(z(1, 19, 3), z(1, 3), z(1, 19, 3), z(19), [0.] * 16, 0.)


def test_keypoint_energy_matches_its_float64_restatement():
    """Bound: the pixel coordinates carry the float32 rounding of ~16 operations on numbers of the size of the image,
    ex = 16 u max(|x|, |cx|, |kx|); the energy term f(r^2) inherits f'(r^2) 2 (|dx| + |dy|) ex plus 16 u of itself, the gradient
    2 f'(r^2) (f / z) (1 + |pc_x / z| + |pc_y / z|) ex for the error of (dx, dy) plus 32 u of itself and of the terms it is the difference of."""
    from selfreconcode_amd import smpl_fit as sf
    cam = sf.make_camera(twin.rodrigues(np.array([[0.1, 3.0, -0.2]]))[0], [0.03, -0.2, 2.5], 648., 650., 271., 268.5)
    T, K, sigma = 5, 19, 100.
    pc = det_array((T, K, 3), 760, 0.6, np.float64) + [0., 0., 2.5]                # camera-frame points 1.9 .. 3.1 in front
    trans = det_array((T, 3), 761, 0.1, np.float64)
    joints = (pc - cam['T']) @ cam['R'].T - trans[:, None]
    x, y, z = (a.numpy() for a in gtwin.project(torch.from_numpy(joints + trans[:, None]), cam))
    off = det_array((T, K, 2), 762, 30.0, np.float64)
    off[3] *= 10.0                                                             # a frame far off: the robust term's flat part
    kp = np.stack([x + off[..., 0], y + off[..., 1], 0.2 + 0.8 * np.abs(det_array((T, K), 763, 1.0, np.float64))], -1)
    kp[0, 3, 2] = 0.0
    kp[1, 4, 0] = np.nan
    kp[2, 5, 2] = np.inf
    joints[4, 6] = (np.array([0.1, 0.1, -0.5]) - cam['T']) @ cam['R'].T - trans[4]        # behind the camera
    jw = np.linspace(0.5, 1.5, K)
    j32, t32, k32, w32 = (np.asarray(a, np.float32) for a in (joints, trans, kp, jw))
    tj, tt = torch.from_numpy(j32.astype(np.float64)).requires_grad_(True), torch.from_numpy(t32.astype(np.float64)).requires_grad_(True)
    cam32 = sf.make_camera(cam['R'].astype(np.float32), cam['T'].astype(np.float32), cam['fx'], cam['fy'], cam['cx'], cam['cy'])
    e64, behind64 = gtwin.keypoint_energy(tj, tt, k32.astype(np.float64), w32.astype(np.float64), cam32, sigma)
    gj64, gt64 = torch.autograd.grad(e64.sum(), [tj, tt])
    energy, g_joints, g_trans, behind = ops.keypoint_energy(_dev(j32), _dev(t32), _dev(k32), _dev(w32), sf.camera_floats(cam32), sigma)
    assert behind.dtype == torch.int32 and behind.cpu().tolist() == [0, 0, 0, 0, 1] and behind64.tolist() == [0, 0, 0, 0, 1]
    g_joints_h = g_joints.cpu().numpy()
    for t, k in ((0, 3), (1, 4), (2, 5), (4, 6)):
        assert not g_joints_h[t, k].any() and not gj64[t, k].any()
    assert np.isfinite(g_joints_h).all() and torch.isfinite(energy).all() and torch.isfinite(g_trans).all()
    # bounds from the float64 quantities
    s = (w32.astype(np.float64) * k32[..., 2].astype(np.float64)) ** 2
    ok = np.isfinite(k32).all(-1) & (k32[..., 2] != 0)
    ok[4, 6] = False
    dx, dy = np.where(ok, x - k32[..., 0], 0.), np.where(ok, y - k32[..., 1], 0.)
    r2 = dx ** 2 + dy ** 2
    fp = np.where(ok, s * (sigma ** 2 / (sigma ** 2 + r2)) ** 2, 0.)
    ex = 16 * U * np.maximum(np.maximum(np.abs(x), np.abs(y)), 600.)
    e_terms = fp * r2 / (sigma ** 2 / (sigma ** 2 + r2))
    e_bound = (fp * 2 * (np.abs(dx) + np.abs(dy)) * ex + 16 * U * e_terms).sum(1)
    e_err = np.abs(energy.cpu().numpy() - e64.detach().numpy())
    print("keypoint energy: error", e_err, "bound", e_bound)
    assert (e_err <= e_bound).all()
    zz = np.where(ok, z, 1.)
    g_mag = 2 * fp * (650. / zz) * (1 + np.abs(pc[..., 0] / zz) + np.abs(pc[..., 1] / zz))
    g_bound = g_mag * ex + 32 * U * g_mag * (np.abs(dx) + np.abs(dy))
    g_err = np.abs(g_joints_h - gj64.numpy()).max(-1)
    print("keypoint gradient: largest error / bound", float((g_err / np.maximum(g_bound, 1e-30)).max()))
    assert (g_err <= g_bound).all()
    gt_err = np.abs(g_trans.cpu().numpy() - gt64.numpy()).max(-1)
    assert (gt_err <= g_bound.sum(1)).all()
    again = ops.keypoint_energy(_dev(j32), _dev(t32), _dev(k32), _dev(w32), sf.camera_floats(cam32), sigma)
    assert all(torch.equal(a, b) for a, b in zip(again, (energy, g_joints, g_trans, behind)))
