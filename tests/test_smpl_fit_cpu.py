"""Host side of the SMPL fit (smpl_fit.py, fit_smpl.py) and the float64 twins the GPU tests lean on (tests/_smplgrad_ref.py): none of
this needs a GPU.

The twin's gradients are checked twice: against the reference's own float64 autograd (tests/golden/smpl_grad.npz, written by
tools/gen_smpl_grad_golden.py) within the reference's recorded float32 error, and against central differences."""
import functools
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import _smpl_ref as twin
import _smplgrad_ref as gtwin
from selfreconcode_amd.synthetic import det_array, synthetic_smpl_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "smpl_grad.npz")))


@functools.lru_cache(maxsize=None)
def _model():
    return synthetic_smpl_model(twin.GOLDEN_NV, twin.GOLDEN_SEED)


def _golden_cotangents():
    from gen_smpl_grad_golden import cotangents, SEED_CV, SEED_CJ
    assert int(_gold()["seed_cv"]) == SEED_CV and int(_gold()["seed_cj"]) == SEED_CJ
    return cotangents(twin.GOLDEN_B, twin.GOLDEN_NV)


def test_twin_gradients_equal_the_references_float64_gradients():
    gold = _gold()
    assert twin.model_sha256(_model()) == str(gold["model_sha256"])
    beta, theta = twin.golden_inputs()
    Cv, Cj = _golden_cotangents()
    got = gtwin.gradients(_model(), beta, theta, Cv, Cj)
    got.update({"avatar_" + k: v for k, v in gtwin.avatar_gradients(_model(), _model()["v_template"], beta, theta, Cv).items()})
    for name in ("g_beta", "g_theta", "gA", "gJ", "avatar_g_Tvs", "avatar_g_beta", "avatar_g_theta"):
        e = float(np.abs(got[name] - gold[name]).max())
        print(f"{name}: twin vs reference float64 {e:.3e} (reference's own float32 error {float(gold['err_' + name]):.3e})")
        assert e <= float(gold["err_" + name]), (name, e)


def test_twin_gradients_match_central_differences():
    model = _model()
    beta, theta = (a.astype(np.float64) for a in twin.golden_inputs(2, seed=5))
    theta[0, 5] = 0.3                                                   # (differences across theta = 0 see the kink of |theta + 1e-8|)
    Cv = det_array((2, twin.GOLDEN_NV, 3), 750, 1.0, np.float64)
    Cj = det_array((2, 19, 3), 751, 1.0, np.float64)
    m = gtwin.Model(model)

    def loss(b, t):
        out = gtwin.forward(m, b, t)
        return float((torch.from_numpy(Cv) * out["verts"]).sum() + (torch.from_numpy(Cj) * out["joints"]).sum())

    g = gtwin.gradients(model, beta, theta, Cv, Cj)
    h = 1e-6
    for name, x, picks in (("g_beta", beta, [(0, 0), (1, 7)]), ("g_theta", theta, [(0, 0, 1), (1, 16, 2), (0, 9, 0)])):
        for idx in picks:
            hi, lo = x.copy(), x.copy()
            hi[idx] += h; lo[idx] -= h
            fd = (loss(hi, theta) - loss(lo, theta)) / (2 * h) if name == "g_beta" else (loss(beta, hi) - loss(beta, lo)) / (2 * h)
            # central differences: truncation h^2 |f'''| / 6 and rounding eps |L| / h ~ 1e-16 * 1e2 / 1e-6
            assert abs(fd - g[name][idx]) <= 1e-6 * max(1.0, abs(fd)), (name, idx, fd, g[name][idx])


def test_keypoint_twin_matches_central_differences_and_masks():
    from selfreconcode_amd import smpl_fit as sf
    cam = sf.make_camera(np.diag([-1., 1., -1.]), [0.03, -0.2, 2.5], 648., 650., 271., 268.5)
    joints = det_array((2, 19, 3), 760, 0.5, np.float64)
    trans = det_array((2, 3), 761, 0.1, np.float64)
    x, y, _ = gtwin.project(torch.from_numpy(joints + trans[:, None]), cam)
    kp = np.stack([x.numpy() + 7.0, y.numpy() - 4.0, np.full((2, 19), 0.8)], -1)
    kp[0, 3, 2] = 0.0
    kp[1, 4, 0] = np.nan
    joints[1, 6, 2] = 3.0                                              # behind the camera (pc_z = -z + 2.5 < 0)
    jw = np.linspace(0.5, 1.5, 19)
    tj, tt = torch.from_numpy(joints).requires_grad_(True), torch.from_numpy(trans).requires_grad_(True)
    e, behind = gtwin.keypoint_energy(tj, tt, kp, jw, cam, 100.)
    gj, gt = torch.autograd.grad(e.sum(), [tj, tt])
    assert behind.tolist() == [0, 1] and torch.isfinite(gj).all() and torch.isfinite(gt).all()
    assert float(gj[0, 3].abs().max()) == 0 and float(gj[1, 4].abs().max()) == 0 and float(gj[1, 6].abs().max()) == 0
    want = (jw[0] * 0.8) ** 2 * 100. ** 2 * 65. / (100. ** 2 + 65.)          # r^2 = 7^2 + 4^2
    assert abs(float(gtwin.keypoint_energy(tj[:1, :1].detach(), tt[:1].detach(), kp[:1, :1], jw[:1], cam, 100.)[0]) - want) <= 1e-9 * want
    h = 1e-6
    for idx in ((0, 0, 0), (1, 9, 2)):
        hi, lo = joints.copy(), joints.copy()
        hi[idx] += h; lo[idx] -= h
        fd = (float(gtwin.keypoint_energy(torch.from_numpy(hi), tt.detach(), kp, jw, cam, 100.)[0].sum())
              - float(gtwin.keypoint_energy(torch.from_numpy(lo), tt.detach(), kp, jw, cam, 100.)[0].sum())) / (2 * h)
        assert abs(fd - float(gj[idx])) <= 1e-5 * max(1.0, abs(fd))


def test_conversion_tables():
    from selfreconcode_amd import smpl_fit as sf
    for fmt, n in (("coco18", 18), ("body25", 25)):
        table = sf.KEYPOINT_TABLES[fmt]
        used = [s for s in table if s >= 0]
        assert len(table) == 19 and table[13] == -1 and len(used) == 18 and len(set(used)) == 18 and all(0 <= s < n for s in used)
        kp = np.zeros((2, n, 3), np.float32)
        kp[..., 0] = np.arange(n); kp[..., 1] = 100 + np.arange(n); kp[..., 2] = 0.5
        out = sf.convert_keypoints(kp, fmt)
        assert out.shape == (2, 19, 3) and out.dtype == np.float32
        assert out[0, 13, 2] == 0                                       # no head top in either layout: confidence 0
        for k, s in enumerate(table):
            if s >= 0:
                assert out[1, k].tolist() == [s, 100 + s, 0.5]
    # left and right are mirror images of each other in both layouts: the model's (R, L) pairs map to the detector's (R, L) pairs
    for fmt, rl in (("coco18", {8: 11, 9: 12, 10: 13, 2: 5, 3: 6, 4: 7, 14: 15, 16: 17}), ("body25", {9: 12, 10: 13, 11: 14, 2: 5, 3: 6, 4: 7, 15: 16, 17: 18})):
        table = sf.KEYPOINT_TABLES[fmt]
        for right, left in ((0, 5), (1, 4), (2, 3), (6, 11), (7, 10), (8, 9), (16, 15), (18, 17)):
            assert rl[table[right]] == table[left], (fmt, right, left)
    ident = np.arange(19 * 3, dtype=np.float32).reshape(1, 19, 3)
    assert np.array_equal(sf.convert_keypoints(ident, "cocoplus"), ident)
    with pytest.raises(ValueError, match="format"):
        sf.convert_keypoints(ident, "mpii")
    with pytest.raises(ValueError, match="coco18"):
        sf.convert_keypoints(ident, "coco18")


def test_read_keypoints_npz_and_openpose(tmp_path):
    from selfreconcode_amd import smpl_fit as sf
    kp = det_array((4, 19, 3), 770, 100.0)
    np.savez(tmp_path / "kp.npz", keypoints=kp)
    assert np.array_equal(sf.read_keypoints(tmp_path / "kp.npz", 3), kp[:3])
    with pytest.raises(ValueError, match="frames"):
        sf.read_keypoints(tmp_path / "kp.npz", 5)
    folder = tmp_path / "openpose"
    folder.mkdir()
    people = {}
    for frame in (2, 10, 1):                                            # (ordered by the integer, not by the string)
        a, b = det_array((25, 3), 771 + frame, 50.0), det_array((25, 3), 781 + frame, 50.0)
        a[:, 2], b[:, 2] = 0.3, 0.6                                     # the second person is the more confident one
        people[frame] = b
        persons = [] if frame == 10 else [{"pose_keypoints_2d": a.reshape(-1).tolist()}, {"pose_keypoints_2d": b.reshape(-1).tolist()}]
        (folder / f"video_{frame:012d}_keypoints.json").write_text(json.dumps({"version": 1.3, "people": persons}))
    got = sf.read_keypoints(folder, 3, "body25")
    assert got.shape == (3, 19, 3)
    assert np.array_equal(got[0], sf.convert_keypoints(people[1][None], "body25")[0])
    assert np.array_equal(got[1], sf.convert_keypoints(people[2][None], "body25")[0])
    assert not got[2].any()                                             # the frame without people: all confidences 0
    with pytest.raises(ValueError, match="frames"):
        sf.read_keypoints(folder, 4, "body25")


def test_stage0_recovers_the_translation_of_a_synthetic_frame():
    """A torso whose four joints lie in a plane parallel to the image plane: every pair obeys the pinhole relation
    (2-D length in focal units) = (3-D length) / depth exactly, and the hip centre lies on the ray through its projection, so the
    closed form is exact up to float64 rounding of ~10 operations on numbers <= 1e3: a relative 1e-12."""
    from selfreconcode_amd import smpl_fit as sf
    q = np.array([0.3, -0.2, 0.9, 0.1])
    cam = sf.make_camera(sf.quat_to_matrix(q), [0.03, -0.2, 2.5], 648., 650., 271., 268.5)
    J0 = det_array((19, 3), 790, 0.4, np.float64)
    J0[[2, 3, 8, 9]] = [[-0.1, -0.3, 0.], [0.12, -0.31, 0.], [-0.2, 0.2, 0.], [0.19, 0.22, 0.]]
    # place the model plane parallel to the image plane: world points = (camera-frame points - T) R^T
    want = np.array([[0.2, -0.1, 0.4], [-0.3, 0.05, 0.1], [0.0, 0.0, 0.0]])
    kp = np.zeros((3, 19, 3))
    trans = np.zeros((3, 3))
    for t in range(3):
        pc = J0 * [1., 1., 0.] + [want[t, 0], want[t, 1], 2.0 + want[t, 2]]      # the torso at one depth
        kp[t, :, 0] = cam['cx'] - cam['fx'] * pc[:, 0] / pc[:, 2]
        kp[t, :, 1] = cam['cy'] - cam['fy'] * pc[:, 1] / pc[:, 2]
        kp[t, :, 2] = 1.0
        hip_c = 0.5 * (pc[2] + pc[3])
        trans[t] = (hip_c - cam['T']) @ cam['R'].T - 0.5 * (J0[2] + J0[3])
    kp[2, [8, 9], 2] = 0.0                                              # frame 2 keeps one pair only: it takes frame 1's value
    got = sf.initial_translation(kp, J0, cam)
    assert np.abs(got[:2] - trans[:2]).max() <= 1e-12 * 1e3
    assert np.array_equal(got[2], got[1])
    with pytest.raises(ValueError, match="no frame"):
        sf.initial_translation(kp[2:], J0, cam)


def test_default_starts_are_the_identity_and_the_half_turn_through_the_camera():
    from selfreconcode_amd import smpl_fit as sf
    cam = sf.make_camera(sf.quat_to_matrix([0.3, -0.2, 0.9, 0.1]), [0., 0., 2.5], 600., 600., 270., 270.)
    starts = sf.default_starts(cam)
    R0, R1 = twin.rodrigues(starts)
    assert np.abs(R0 - cam['R']).max() <= 1e-7 and np.abs(R1 - cam['R'] @ np.diag([-1., 1., -1.])).max() <= 1e-7
    assert np.abs(sf.matrix_to_axis_angle(np.eye(3))).max() == 0


def _copy_scene(tmp_path):
    dst = tmp_path / "scene"
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "scene_folder"), dst)
    os.remove(dst / "smpl_rec.npz")
    return dst


def _result(F):
    return {"poses": det_array((F, 24, 3), 795, 0.3), "shape": det_array((10,), 796, 1.0), "trans": det_array((F, 3), 797, 0.2), "gender": "female",
            "reproj": np.linspace(0.5, 2.5, F), "behind": np.zeros(F, np.int32), "history": np.array([10., 1.]), "start": 1}


def test_written_file_is_read_back_by_read_scene_folder(tmp_path):
    from selfreconcode_amd import fit_smpl
    from selfreconcode_amd.dataset.dataset import read_scene_folder
    scene = _copy_scene(tmp_path)
    F = fit_smpl.count_frames(str(scene))
    assert F == 12
    res = _result(F)
    fit_smpl.write_smpl_rec(str(scene / "smpl_rec.npz"), res)
    with np.load(scene / "smpl_rec.npz") as data:
        assert data["poses"].dtype == np.float32 and data["poses"].shape == (F, 24, 3) and data["shape"].shape == (10,) and data["trans"].shape == (F, 3)
    got = read_scene_folder(scene)
    assert np.array_equal(got["poses"], res["poses"]) and np.array_equal(got["trans"], res["trans"]) and np.array_equal(got["shape"], res["shape"])
    assert got["gender"] == "female" and got["frame_num"] == F
    report = fit_smpl.write_report(str(scene / "smpl_fit.json"), res)
    assert json.loads((scene / "smpl_fit.json").read_text()) == report
    assert len(report["frames"]) == F and report["summary"]["worst_frames"][0] == F - 1 and abs(report["summary"]["reproj_mean"] - 1.5) < 1e-12


def test_overwrite_refusal_and_argument_errors(tmp_path, capsys):
    from selfreconcode_amd import fit_smpl
    scene = _copy_scene(tmp_path)
    target = scene / "smpl_rec.npz"
    fit_smpl.write_smpl_rec(str(target), _result(12))
    with pytest.raises(FileExistsError, match="smpl_rec.npz"):
        fit_smpl.write_smpl_rec(str(target), _result(12))
    fit_smpl.write_smpl_rec(str(target), _result(12), force=True)
    np.savez(tmp_path / "kp.npz", keypoints=np.zeros((12, 19, 3), np.float32))
    with pytest.raises(FileExistsError, match="smpl_rec.npz"):          # the command refuses before it touches a GPU
        fit_smpl.main(["--data", str(scene), "--keypoints", str(tmp_path / "kp.npz")])
    for argv in (["--keypoints", str(tmp_path / "kp.npz")], ["--data", str(scene)],
                 ["--data", str(tmp_path / "nowhere"), "--keypoints", str(tmp_path / "kp.npz")],
                 ["--data", str(tmp_path), "--keypoints", str(tmp_path / "kp.npz")],
                 ["--data", str(scene), "--keypoints", str(tmp_path / "missing.npz")],
                 ["--data", str(scene), "--keypoints", str(tmp_path / "kp.npz"), "--format", "mpii"],
                 ["--data", str(scene), "--keypoints", str(tmp_path / "kp.npz"), "--init", str(tmp_path / "none.npz")]):
        with pytest.raises(SystemExit) as e:
            fit_smpl.parse_args(argv)
        assert e.value.code == 2
    capsys.readouterr()
    with pytest.raises(ValueError, match="shape"):
        fit_smpl.write_smpl_rec(str(tmp_path / "x.npz"), dict(_result(12), shape=np.zeros(9)))
    os.remove(scene / "imgs" / "3.png")
    with pytest.raises(ValueError, match="count 0, 1, 2"):
        fit_smpl.count_frames(str(scene))


def test_twin_fit_converges_on_the_small_scene():
    """The scene of tests/test_smpl_fit_gpu.py: the float64 restatement of the loop must itself end below a pixel, or the GPU test's
    condition (at most twice the twin's error plus 0.05 px) would say nothing."""
    import _smplfit_scene as scene
    s = scene.scene()
    out = scene.twin_fit()
    print(f"twin: start {out['start']}, reprojection mean {out['reproj'].mean():.4f} px, max {out['reproj'].max():.4f} px, "
          f"energy {out['history'][0]:.3e} -> {out['history'][-1]:.3e}")
    assert out["start"] == s["true_start"] == 1
    assert out["reproj"].mean() < 1.0
