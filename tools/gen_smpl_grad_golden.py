"""Writes tests/golden/smpl_grad.npz: gradients of the reference's OWN SMPL class (smpl_pytorch/SMPL.py, imported unmodified through
oracle.ref_harness, CPU) on synthetic.synthetic_smpl_model(200, seed) with the golden inputs of tests/_smpl_ref.py, by torch.autograd:

  forward:  L = sum Cv verts + sum Cj joints      -> g_beta, g_theta, and the cotangents the class exposes as attributes: gA (of smpl.A,
                                                      rows 0..2) and gJ (of smpl.J)
  avatar:   L = sum Cv avatar(Tvs, beta, theta)   -> avatar_g_Tvs, avatar_g_beta, avatar_g_theta

each evaluated twice: in float32, and in float64 (smpl.double() under torch.set_default_dtype(torch.float64): the reference's util.py
builds torch.ones / torch.zeros without a dtype).  The file keeps the float64 gradients and err_<name> = the largest difference
between the reference's float32 and float64 gradient; Cv, Cj are det_array at the recorded seeds.  Needs the reference checkout; only
data goes into the file.

    python tools/gen_smpl_grad_golden.py
"""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import _smpl_ref as twin  # noqa: E402
from gen_smpl_golden import write_model_txt  # noqa: E402
from selfreconcode_amd.synthetic import det_array, synthetic_smpl_model  # noqa: E402

SEED_CV, SEED_CJ = 740, 741


def cotangents(B, nv, nk=19):
    """(Cv [B,nv,3], Cj [B,nk,3]) float32, scaled so that a sum over the vertices keeps its size when nv changes."""
    s = np.float32(np.sqrt(twin.GOLDEN_NV / nv))
    return det_array((B, nv, 3), SEED_CV, 1.0) * s, det_array((B, nk, 3), SEED_CJ, 1.0)


def _grads(smpl, beta, theta, Tvs, Cv, Cj, dtype):
    tb = torch.from_numpy(beta).to(dtype).requires_grad_(True)
    tt = torch.from_numpy(theta).to(dtype).requires_grad_(True)
    verts, joints, _ = smpl(tb, tt, get_skin=True)
    L = (torch.from_numpy(Cv).to(dtype) * verts).sum() + (torch.from_numpy(Cj).to(dtype) * joints).sum()
    g = torch.autograd.grad(L, [tb, tt, smpl.A, smpl.J])
    out = {"g_beta": g[0], "g_theta": g[1], "gA": g[2][:, :, :3, :].reshape(-1, 24, 12), "gJ": g[3]}
    tv = torch.from_numpy(Tvs).to(dtype).requires_grad_(True)
    La = (torch.from_numpy(Cv).to(dtype) * smpl.avatar(tv, tb, tt)).sum()
    g = torch.autograd.grad(La, [tv, tb, tt])
    out.update(avatar_g_Tvs=g[0], avatar_g_beta=g[1], avatar_g_theta=g[2])
    return {k: v.detach().double().numpy() for k, v in out.items()}


def main():
    from oracle.ref_harness import load_reference
    ref = load_reference().Deformer
    if not hasattr(np, "float"):
        np.float = float                                   # the reference's constructor still spells it that way
    model = synthetic_smpl_model(twin.GOLDEN_NV, twin.GOLDEN_SEED)
    beta, theta = twin.golden_inputs()
    Cv, Cj = cotangents(twin.GOLDEN_B, twin.GOLDEN_NV)
    Tvs = model["v_template"]
    out = {"model_sha256": np.array(twin.model_sha256(model)), "seed_cv": np.int64(SEED_CV), "seed_cj": np.int64(SEED_CJ)}
    with tempfile.TemporaryDirectory() as tmp:
        stem = os.path.join(tmp, "synthetic_smpl")
        write_model_txt(model, stem)
        g32 = _grads(ref.SMPL(stem, obj_saveable=True), beta, theta, Tvs, Cv, Cj, torch.float32)
        torch.set_default_dtype(torch.float64)
        try:
            g64 = _grads(ref.SMPL(stem, obj_saveable=True).double(), beta, theta, Tvs, Cv, Cj, torch.float64)
        finally:
            torch.set_default_dtype(torch.float32)
    for name, g in g64.items():
        e = np.abs(g32[name] - g).max()
        out[name] = g
        out["err_" + name] = np.float64(e)
        print(f"{name} {g.shape}: reference float32 vs float64 {e:.3e} (largest value {np.abs(g).max():.3f})")
    path = os.path.join(ROOT, "tests", "golden", "smpl_grad.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
