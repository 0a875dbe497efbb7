"""The small fitting scene shared by tests/test_smpl_fit_cpu.py and tests/test_smpl_fit_gpu.py, and its float64 twin fit (computed once
per process): nv = 200, F = SMPL_BATCH_TILE + 1 frames, a 540 x 540 camera like tests/golden/camera.npz's.  Ground truth: beta in
+-1, body poses that vary smoothly over the frames with joint angles up to 0.4 rad, the root facing the camera (the half turn of
smpl_fit.default_starts) with a small smooth sway, the body 2-3 units in front of the camera.  The keypoints are the twin's float64
projections; three confidences are 0."""
import functools
import os

import numpy as np
import torch

import _smpl_ref as twin
import _smplgrad_ref as gtwin
from selfreconcode_amd.synthetic import det_array, synthetic_smpl_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV, F = 200, 9
# (iterations, lr, l_theta, l_beta, l_s): stage 1, then three rounds of stage 2 -- chosen so that the float64 twin ends below a pixel (0.27 px) in a few seconds on the CPU
STAGES = ((30, 0.05, 0., 0., 100.), (60, 0.03, 10., 10., 100.), (80, 0.01, 1., 1., 10.), (60, 0.004, 0.1, 0.1, 1.))


@functools.lru_cache(maxsize=None)
def model():
    return synthetic_smpl_model(NV, twin.GOLDEN_SEED)


@functools.lru_cache(maxsize=None)
def scene():
    from selfreconcode_amd import ops, smpl_fit as sf
    assert F == ops.SMPL_BATCH_TILE + 1
    with np.load(os.path.join(ROOT, "tests", "golden", "camera.npz")) as data:
        cam = sf.make_camera(data["R"], data["T"], data["focal"][0], data["focal"][1], data["princ"][0], data["princ"][1])
    t = np.linspace(0., 1., F)[:, None, None]
    amp, phase = det_array((1, 24, 3), 801, 0.4, np.float64), det_array((1, 24, 3), 802, np.pi, np.float64)
    poses = amp * np.sin(2 * np.pi * 0.5 * t + phase)                   # |angle component| <= 0.4, half a period over the sequence
    starts = sf.default_starts(cam)
    poses[:, 0] = starts[1] + 0.1 * np.sin(2 * np.pi * 0.5 * t[:, 0] + phase[0, 0])
    beta = det_array((1, 10), 803, 1.0, np.float64)
    tt = t[:, 0, 0]
    trans = np.stack([0.1 * np.sin(2 * np.pi * tt), 0.05 * np.cos(2 * np.pi * tt), -0.1 + 0.3 * np.sin(np.pi * tt)], 1)
    m = gtwin.Model(model())
    joints = gtwin.forward(m, torch.from_numpy(beta).expand(F, -1), torch.from_numpy(poses))["joints"] + torch.from_numpy(trans).view(F, 1, 3)
    x, y, z = gtwin.project(joints, cam)
    assert float(z.min()) > 1.5 and float(z.max()) < 3.5
    kp = np.stack([x.numpy(), y.numpy(), np.ones((F, 19))], -1)
    for f, k in ((0, 6), (4, 13), (8, 1)):
        kp[f, k, 2] = 0.0
    return {"camera": cam, "poses": poses, "beta": beta[0], "trans": trans, "keypoints": kp, "joints3d": joints.numpy(), "true_start": 1}


@functools.lru_cache(maxsize=None)
def twin_fit():
    s = scene()
    return gtwin.fit_sequence(model(), s["keypoints"], s["camera"], STAGES)


@functools.lru_cache(maxsize=None)
def twin_fit_3d():
    """The 3-D term alone: 2-D weights at zero, started from the result of stages 0 and 1 (so that the 3-D term has work to do)."""
    s = scene()
    return gtwin.fit_sequence(model(), s["keypoints"], s["camera"], STAGES[:2], joints3d=s["joints3d"], joint_weights=np.zeros(19), init=init_3d())


def init_3d():
    """A start for the 3-D runs: the truth disturbed by a fixed smooth error."""
    s = scene()
    return {"poses": s["poses"] + det_array((F, 24, 3), 810, 0.15, np.float64), "shape": np.zeros(10), "trans": s["trans"] + 0.05}
