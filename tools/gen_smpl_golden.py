"""Writes tests/golden/smpl.npz: the reference's OWN SMPL class (smpl_pytorch/SMPL.py, imported unmodified through
oracle.ref_harness, CPU, float32) on synthetic.synthetic_smpl_model(200, seed) written to a temporary `<stem>.txt` -- outputs only
(verts, joints, Rs, J, J_transformed, A and the avatar result), each with the reference's float32 error against the float64 twin of
tests/_smpl_ref.py, and the SHA-256 of the model arrays.  Needs the reference checkout; only data goes into the file.

    python tools/gen_smpl_golden.py
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _smpl_ref as twin  # noqa: E402
from selfreconcode_amd.synthetic import synthetic_smpl_model  # noqa: E402


def write_model_txt(model, stem):
    with open(stem + ".txt", "w") as fh:
        json.dump({k: np.asarray(v).tolist() for k, v in model.items()}, fh)


def main():
    from oracle.ref_harness import load_reference
    ref = load_reference().Deformer
    if not hasattr(np, "float"):
        np.float = float                                   # the reference's constructor still spells it that way
    model = synthetic_smpl_model(twin.GOLDEN_NV, twin.GOLDEN_SEED)
    beta, theta = twin.golden_inputs()
    out = {"model_sha256": np.array(twin.model_sha256(model)), "outputs": np.array(twin.OUTPUTS)}
    with tempfile.TemporaryDirectory() as tmp:
        stem = os.path.join(tmp, "synthetic_smpl")
        write_model_txt(model, stem)
        for joint_type in ("cocoplus", "lsp"):
            smpl = ref.SMPL(stem, joint_type=joint_type, obj_saveable=True)
            tb, tt = torch.from_numpy(beta), torch.from_numpy(theta)
            with torch.no_grad():
                verts, joints, Rs = smpl(tb, tt, get_skin=True)
                got = {"verts": verts, "joints": joints, "Rs": Rs, "J": smpl.J, "J_transformed": smpl.J_transformed, "A": smpl.A}
                J = smpl.skeleton(tb, False)
                assert torch.equal(J, smpl.J)
                got["avatar"] = smpl.avatar(torch.from_numpy(model["v_template"]), tb, tt)
            want = twin.forward(model, beta, theta, joint_type=joint_type, Tvs=model["v_template"])
            if joint_type == "lsp":
                e = np.abs(got["joints"].numpy() - want["joints"]).max()
                out.update(joints_lsp=got["joints"].numpy(), err_joints_lsp=np.float64(e))
                print(f"joints (lsp) {tuple(got['joints'].shape)}: reference float32 vs float64 twin {e:.3e}")
                continue
            for name in twin.OUTPUTS:
                g = got[name].numpy()
                assert g.dtype == np.float32 and g.shape == want[name].shape, (name, g.dtype, g.shape, want[name].shape)
                e = np.abs(g - want[name]).max()
                out[name] = g
                out["err_" + name] = np.float64(e)
                print(f"{name} {g.shape}: reference float32 vs float64 twin {e:.3e} (largest value {np.abs(want[name]).max():.3f})")
    path = os.path.join(ROOT, "tests", "golden", "smpl.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
