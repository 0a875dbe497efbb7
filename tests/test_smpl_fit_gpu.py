"""smpl_fit.fit_sequence on the GPU against its float64 restatement (tests/_smplgrad_ref.py::fit_sequence, run once on the CPU on the
same scene, tests/_smplfit_scene.py): nv = 200, F = SMPL_BATCH_TILE + 1, a 540 x 540 camera.

Condition: the GPU's final mean reprojection error is at most twice the twin's plus 0.05 px (a float32 Adam trajectory drifts from
the float64 one); with joints3d given and the 2-D weights at zero the same rule holds for the mean 3-D joint error, which must also
fall below the start's.  Measured on an MI355X: 0.2728 px on the GPU, 0.2728 px for the twin; 3-D error 0.00324 for both from a start
of 0.09369 (profiles/smpl_fit.md).
"""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import _smplfit_scene as scene
from selfreconcode_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _smpl():
    from selfreconcode_amd.smpl_pytorch import DifferentiableSMPL
    return DifferentiableSMPL(scene.model(), obj_saveable=True).to(DEV)


def _joints3d(smpl, out):
    with torch.no_grad():
        F = out["poses"].shape[0]
        beta = torch.from_numpy(out["shape"]).to(DEV).view(1, -1).expand(F, -1).contiguous()
        joints = smpl(beta, torch.from_numpy(out["poses"]).to(DEV))
    return joints.double().cpu().numpy() + out["trans"].astype(np.float64)[:, None]


def test_fit_recovers_the_scene_like_its_float64_restatement():
    from selfreconcode_amd import smpl_fit as sf
    s = scene.scene()
    assert scene.F == ops.SMPL_BATCH_TILE + 1
    want = scene.twin_fit()
    smpl = _smpl()
    got = sf.fit_sequence(smpl, s["keypoints"], s["camera"], stages=scene.STAGES)
    assert got["poses"].shape == (scene.F, 24, 3) and got["poses"].dtype == np.float32 and got["shape"].shape == (10,) and got["trans"].shape == (scene.F, 3)
    assert got["history"].shape == (2 * scene.STAGES[0][0] + sum(st[0] for st in scene.STAGES[1:]),) and np.isfinite(got["history"]).all()
    assert got["start"] == want["start"] == s["true_start"]                   # stage 0 + 1 picks the half turn the truth has
    assert not got["behind"].any()
    e_gpu, e_twin = float(got["reproj"].mean()), float(want["reproj"].mean())
    print(f"reprojection error: GPU {e_gpu:.4f} px, float64 twin {e_twin:.4f} px; energy {got['history'][0]:.3e} -> {got['history'][-1]:.3e}")
    assert e_twin < 1.0
    assert e_gpu <= 2 * e_twin + 0.05
    again = sf.fit_sequence(smpl, s["keypoints"], s["camera"], stages=scene.STAGES)
    for key in ("poses", "shape", "trans", "reproj", "history", "behind"):
        assert np.array_equal(again[key], got[key]), key                        # no random numbers, no atomics: bit for bit


def test_fit_to_3d_joints_with_the_2d_weights_at_zero():
    from selfreconcode_amd import smpl_fit as sf
    s = scene.scene()
    want = scene.twin_fit_3d()
    smpl = _smpl()
    init = {k: np.asarray(v, np.float32) for k, v in scene.init_3d().items()}
    start = _joints3d(smpl, init)
    got = sf.fit_sequence(smpl, s["keypoints"], s["camera"], joints3d=s["joints3d"], joint_weights=np.zeros(19), init=init, stages=scene.STAGES[:2])
    err = lambda J: float(np.linalg.norm(J - s["joints3d"], axis=-1).mean())          # noqa: E731
    e_start, e_gpu, e_twin = err(start), err(_joints3d(smpl, got)), err(want["joints3d"])
    print(f"mean 3-D joint error: start {e_start:.5f}, GPU {e_gpu:.5f}, float64 twin {e_twin:.5f}")
    assert e_twin < e_start and e_gpu < e_start
    assert e_gpu <= 2 * e_twin + 0.05 * 2.5 / 650.                            # (0.05 px at the scene's depth and focal length, in world units)


def test_one_start_given_as_a_flat_vector():
    from selfreconcode_amd import smpl_fit as sf
    s = scene.scene()
    stages = ((4, 0.05, 0., 0., 100.), (3, 0.01, 1., 1., 10.))
    one = sf.default_starts(s["camera"])[1]                                     # [3], not [1,3]
    got = sf.fit_sequence(_smpl(), s["keypoints"], s["camera"], stages=stages, starts=one)
    assert got["history"].shape == (4 + 3,) and np.isfinite(got["history"]).all() and got["start"] == 0
    both = sf.fit_sequence(_smpl(), s["keypoints"], s["camera"], stages=stages, starts=[one.tolist(), one.tolist()])
    assert both["history"].shape == (2 * 4 + 3,) and both["start"] == 0         # equal energies: the first
    assert np.array_equal(both["history"][:4], got["history"][:4]) and np.array_equal(both["poses"], got["poses"])


def test_the_command_writes_a_file_scene_dataset_opens(tmp_path):
    from gen_smpl_golden import write_model_txt
    from selfreconcode_amd import fit_smpl
    from selfreconcode_amd.dataset.dataset import SceneDataset
    folder = tmp_path / "scene"
    shutil.copytree(os.path.join(ROOT, "tests", "golden", "scene_folder"), folder)
    os.remove(folder / "smpl_rec.npz")
    models = tmp_path / "models"
    models.mkdir()
    write_model_txt(scene.model(), str(models / "neutral_smpl_with_cocoplus_reg"))
    # keypoints: the projections of a body the folder's own camera sees 2.2 units away, in OpenPose's BODY-25 files
    from selfreconcode_amd import smpl_fit as sf
    import _smplgrad_ref as gtwin
    cam = sf.read_camera(folder / "camera.npz")
    F = fit_smpl.count_frames(str(folder))
    poses = np.zeros((F, 24, 3))
    poses[:, 0] = sf.default_starts(cam)[1]
    trans = np.tile((np.array([0., 0., 2.2]) - cam['T']) @ cam['R'].T, (F, 1))
    m = gtwin.Model(scene.model())
    J = gtwin.forward(m, torch.zeros((F, 10), dtype=torch.float64), torch.from_numpy(poses))["joints"] + torch.from_numpy(trans)[:, None]
    x, y, z = gtwin.project(J, cam)
    assert float(z.min()) > 1.0
    table = sf.KEYPOINT_TABLES["body25"]
    kdir = tmp_path / "openpose"
    kdir.mkdir()
    for f in range(F):
        person = np.zeros((25, 3))
        for k, src in enumerate(table):
            if src >= 0:
                person[src] = [float(x[f, k]), float(y[f, k]), 0.9]
        (kdir / f"clip_{f:06d}_keypoints.json").write_text(json.dumps({"people": [{"pose_keypoints_2d": person.reshape(-1).tolist()}]}))
    lines = []
    argv = ["--gpu-ids", "0", "--data", str(folder), "--keypoints", str(kdir), "--format", "body25", "--model-dir", str(models)]
    result = fit_smpl.main(argv, out=lines.append)
    assert len(lines) == 1 and "smpl_rec.npz" in lines[0] and result["poses"].shape == (F, 24, 3)
    report = json.loads((folder / "smpl_fit.json").read_text())
    assert len(report["frames"]) == F and report["summary"]["behind_total"] == 0
    print(lines[0])
    ds = SceneDataset(str(folder), device=DEV)
    assert ds.frame_num == F and ds.gender == "neutral"
    assert torch.equal(ds.poses.cpu(), torch.from_numpy(result["poses"])) and torch.equal(ds.trans.cpu(), torch.from_numpy(result["trans"]))
    assert torch.equal(ds.shape.cpu(), torch.from_numpy(result["shape"]))
    with pytest.raises(FileExistsError, match="smpl_rec.npz"):
        fit_smpl.main(argv, out=lines.append)
    os.remove(folder / "smpl_fit.json")
    elsewhere = tmp_path / "elsewhere"
    elsewhere.mkdir()
    again = fit_smpl.main(argv + ["--out", str(elsewhere / "rec.npz")], out=lines.append)
    assert (elsewhere / "rec.npz").is_file() and (folder / "smpl_fit.json").is_file() and not (elsewhere / "smpl_fit.json").exists()
    assert np.array_equal(again["poses"], result["poses"])
