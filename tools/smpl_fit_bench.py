"""Times one step of the SMPL fit -- forward, energy, backward, FusedAdam -- with the body model on the kernels (DifferentiableSMPL,
csrc/smpl.hip + csrc/smpl_grad.hip) against the SAME step with the body model composed from torch operators on the GPU
(tests/_smplgrad_ref.py in float32: the obvious alternative), on synthetic_smpl_model(nv) at the real body's size.  Everything else
in the step (the keypoint energy kernel, the priors, the optimiser) is shared.  Seconds of warm-up first (the first launches load
code objects and the clocks ramp), then the two versions alternate, so that a drift of the machine shows as spread, not as a
difference.  Prints one JSON line; needs a GPU.

    python tools/smpl_fit_bench.py [--nv 6890] [--frames 64] [--warmup-seconds 3] [--seconds 2] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _smplgrad_ref as composed  # noqa: E402
from selfreconcode_amd import smpl_fit as sf  # noqa: E402
from selfreconcode_amd.optim import FusedAdam  # noqa: E402
from selfreconcode_amd.smpl_pytorch import DifferentiableSMPL  # noqa: E402
from selfreconcode_amd.synthetic import det_tensor, synthetic_smpl_model  # noqa: E402


class Step:
    """One optimisation step of stage 2 on its own copy of the parameters; `body(beta [F,10], theta [F,24,3]) -> joints [F,19,3]`."""

    def __init__(self, body, F, kp, cam, dev):
        self.body, self.F, self.kp, self.cam = body, F, kp, cam
        self.root = (det_tensor((F, 3), 11, 0.3).to(dev)).requires_grad_(True)
        self.pose = (det_tensor((F, 23, 3), 12, 0.3).to(dev)).requires_grad_(True)
        self.trans = (det_tensor((F, 3), 13, 0.1).to(dev)).requires_grad_(True)
        self.beta = (det_tensor((1, 10), 14, 0.5).to(dev)).requires_grad_(True)
        self.jw = torch.ones(19, device=dev)
        self.opt = FusedAdam([self.root, self.pose, self.trans, self.beta], lr=1e-4)

    def __call__(self):
        F = self.F
        self.opt.zero_grad(set_to_none=True)
        theta = torch.cat([self.root.view(F, 1, 3), self.pose], 1)
        joints = self.body(self.beta.expand(F, -1), theta)
        E = sf.keypoint_energy(joints, self.trans, self.kp, self.jw, self.cam, 100.)[0].sum()
        J3 = joints + self.trans.view(F, 1, 3)
        E = E + 10. * (self.pose ** 2).sum() + 10. * (self.beta ** 2).sum() + 1000. * ((J3[1:] - J3[:-1]) ** 2).sum()
        E.backward()
        self.opt.step()
        return E


def warm(fn, seconds):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()


def timed(fn, seconds):
    """Mean time per call in microseconds: device events around a window of about `seconds` of back-to-back calls."""
    fn(); torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    calls = max(10, min(20000, int(seconds / max(time.perf_counter() - t0, 1e-6))))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    stop.record(); torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e3 / calls, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nv", type=int, default=6890)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup-seconds", type=float, default=3.0)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("smpl_fit_bench: no GPU (a CPU run measures nothing about it)")
    dev, F = "cuda:0", args.frames
    model = synthetic_smpl_model(args.nv, 0)
    smpl = DifferentiableSMPL(model).to(dev)
    m32 = composed.Model(model, dtype=torch.float32, device=dev)
    camera = sf.make_camera(np.diag([-1., 1., -1.]), [0.03, -0.2, 2.5], 648., 650., 271., 268.5)
    cam = sf.camera_floats(camera)
    kp = torch.cat([270. + 100. * det_tensor((F, 19, 2), 15, 1.0), torch.ones(F, 19, 1)], -1).to(dev)
    kernels = Step(lambda b, t: smpl(b, t), F, kp, cam, dev)
    torch_ops = Step(lambda b, t: composed.forward(m32, b, t)["joints"], F, kp, cam, dev)
    # the two steps compute the same thing: same energy on the same parameters (before either has moved)
    e_k, e_t = float(kernels()), float(torch_ops())
    warm(kernels, args.warmup_seconds); warm(torch_ops, args.warmup_seconds)
    k_us, t_us, calls = [], [], 0
    for _ in range(args.rounds):
        us, calls = timed(kernels, args.seconds); k_us.append(us)
        us, _ = timed(torch_ops, args.seconds); t_us.append(us)
    # the two adjoint kernels that do the work, alone
    from selfreconcode_amd import ops
    with torch.no_grad():
        beta = det_tensor((F, 10), 1, 1.5).to(dev)
        theta = det_tensor((F, 24, 3), 2, 0.6).to(dev)
        J, v_shaped = smpl.skeleton(beta, True)
        Rs, feature, _, A = ops.smpl_pose(J, smpl.parents, theta=theta)
        gV = det_tensor((F, args.nv, 3), 3, 1.0).to(dev)
        skin_us, _ = timed(lambda: ops.smpl_skin_bwd(v_shaped, smpl.weight[0], A, gV, smpl.posedirs, feature), 1.0)
        _, gA, g_feature = ops.smpl_skin_bwd(v_shaped, smpl.weight[0], A, gV, smpl.posedirs, feature)
        pose_us, _ = timed(lambda: ops.smpl_pose_bwd(Rs, J, A, smpl.parents, theta=theta, gA=gA, g_feature=g_feature), 1.0)
    tiles = -(-F // ops.SMPL_BATCH_TILE)
    streamed = tiles * (smpl.posedirs.numel() + smpl.weight.numel()) * 4 + 3 * F * args.nv * 12          # posedirs + weights per tile; rest, gV in, g_rest out
    # the body model's own launches, per step: forward 6 (shape, 2 x 2 regress, pose, skin), backward 7 (regress, skin x 2, pose, regress, shape x 2)
    print(json.dumps({"nv": args.nv, "frames": F, "first_energy_kernels": e_k, "first_energy_torch": e_t,
                      "skin_bwd_us": round(skin_us, 1), "skin_bwd_GB_per_s": round(streamed / skin_us / 1e3, 1), "pose_bwd_us": round(pose_us, 1),
                      "kernels_step_us": [round(u, 1) for u in k_us], "torch_step_us": [round(u, 1) for u in t_us],
                      "kernels_step_us_median": round(float(np.median(k_us)), 1), "torch_step_us_median": round(float(np.median(t_us)), 1),
                      "torch_over_kernels": round(float(np.median(t_us) / np.median(k_us)), 2), "timed_calls_per_window": calls}), flush=True)


if __name__ == "__main__":
    main()
