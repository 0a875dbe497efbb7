"""Host-side checks of the SMPL body model: the float64 twin agrees with what the golden generator recorded from the reference's
own class, the three loader forms give equal buffers, a model entry that is no plain array is named, a missing model directory is
reported, and the synthetic model is still the one the golden file was made from.  Nothing computes on the CPU."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

import _smpl_ref as twin
from selfreconcode_amd.synthetic import SMPL_PARENTS, synthetic_smpl_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "smpl.npz")))


@pytest.fixture(scope="module")
def model():
    return synthetic_smpl_model(twin.GOLDEN_NV, twin.GOLDEN_SEED)


def test_synthetic_model_is_the_one_the_golden_file_was_made_from(gold, model):
    assert twin.model_sha256(model) == str(gold["model_sha256"])
    nv = twin.GOLDEN_NV
    assert model["kintree_table"][0].tolist() == SMPL_PARENTS
    assert model["weights"].shape == (nv, 24) and np.abs(model["weights"].sum(1) - 1).max() <= 1e-6 and model["weights"].min() >= 0
    assert float(np.median(model["weights"].max(1))) > 0.5                                 # peaked
    for name, k in (("J_regressor", 24), ("cocoplus_regressor", 19)):
        assert model[name].shape == (nv, k) and model[name].min() >= 0 and np.abs(model[name].sum(0) - 1).max() <= 1e-5
    assert model["shapedirs"].shape == (nv, 3, 10) and 0.02 < np.abs(model["shapedirs"]).max() <= 0.03
    assert model["posedirs"].shape == (nv, 3, 207) and 0.005 < np.abs(model["posedirs"]).max() <= 0.01
    assert model["f"].shape[1] == 3 and model["f"].max() < nv and model["f"].min() >= 0
    again = synthetic_smpl_model(twin.GOLDEN_NV, twin.GOLDEN_SEED)
    assert all(np.array_equal(model[k], again[k]) for k in model)
    assert twin.model_sha256(synthetic_smpl_model(twin.GOLDEN_NV, twin.GOLDEN_SEED + 1)) != str(gold["model_sha256"])


def test_twin_matches_the_golden_within_the_recorded_reference_error(gold, model):
    beta, theta = twin.golden_inputs()
    want = twin.forward(model, beta, theta, Tvs=model["v_template"])
    assert [str(n) for n in gold["outputs"]] == list(twin.OUTPUTS)
    for name in twin.OUTPUTS:
        assert gold[name].dtype == np.float32 and gold[name].shape == want[name].shape
        e = np.abs(gold[name] - want[name]).max()
        print(f"{name}: golden vs twin {e:.3e}, recorded {float(gold['err_' + name]):.3e}")
        assert abs(e - float(gold["err_" + name])) <= 1e-12
        assert float(gold["err_" + name]) < 2e-6                                           # a float32 evaluation, not another function
    lsp = twin.forward(model, beta, theta, joint_type='lsp')["joints"]
    assert abs(np.abs(gold["joints_lsp"] - lsp).max() - float(gold["err_joints_lsp"])) <= 1e-12
    assert np.array_equal(gold["joints_lsp"], gold["joints"][:, :14])
    # theta = 0 goes through the 1e-8 route to the identity
    R0 = twin.rodrigues(np.zeros((2, 3)))
    assert np.abs(R0 - np.eye(3)).max() <= 1e-12


def _buffers(smpl):
    return {k: v.clone() for k, v in smpl.state_dict().items()}


def test_loader_forms_give_equal_buffers(tmp_path, model):
    from selfreconcode_amd.smpl_pytorch import SMPL
    with open(tmp_path / "m.txt", "w") as fh:
        json.dump({k: np.asarray(v).tolist() for k, v in model.items()}, fh)
    np.savez(tmp_path / "n.npz", **model)
    with open(tmp_path / "p.pkl", "wb") as fh:
        pickle.dump(dict(model), fh)
    a = SMPL(model, obj_saveable=True)
    want = _buffers(a)
    assert {'v_template', 'shapedirs', 'J_regressor', 'posedirs', 'joint_regressor', 'weight'} <= set(want)
    nv = twin.GOLDEN_NV
    assert a.shapedirs.shape == (10, 3 * nv) and a.posedirs.shape == (207, 3 * nv) and a.weight.shape == (1, nv, 24)
    assert a.parents.tolist() == SMPL_PARENTS and a.faces == model["f"].tolist() and a.size == [nv, 3]
    for other in (SMPL(str(tmp_path / "m")), SMPL(str(tmp_path / "n.npz")), SMPL(str(tmp_path / "p"))):
        got = _buffers(other)
        assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
        assert other.faces is None and other.parents.tolist() == SMPL_PARENTS
    assert SMPL(model, joint_type='lsp').joint_regressor.shape == (nv, 14)
    assert torch.equal(SMPL(model, joint_type='lsp').joint_regressor, a.joint_regressor[:, :14])
    with pytest.raises(FileNotFoundError):
        SMPL(str(tmp_path / "absent"))


class _Opaque:
    """What an entry of a body-model pickle looks like when it was saved through an array wrapper."""


def test_pickle_with_an_object_entry_names_it(tmp_path, model):
    from selfreconcode_amd.smpl_pytorch import SMPL
    bad = dict(model)
    bad["posedirs"] = _Opaque()
    with open(tmp_path / "bad.pkl", "wb") as fh:
        pickle.dump(bad, fh)
    with pytest.raises(TypeError, match="'posedirs' is not a plain array"):
        SMPL(str(tmp_path / "bad"))


def test_pickle_that_needs_a_missing_package_gets_the_same_advice(tmp_path, model):
    """The official files hold array-wrapper objects of a package that need not be installed: unpickling itself fails then."""
    import sys
    import types
    from selfreconcode_amd.smpl_pytorch import SMPL
    mod = types.ModuleType("array_wrapper_not_installed")
    mod.Wrapped = type("Wrapped", (), {"__module__": "array_wrapper_not_installed"})
    sys.modules[mod.__name__] = mod
    try:
        bad = dict(model)
        bad["v_template"] = mod.Wrapped()
        with open(tmp_path / "wrapped.pkl", "wb") as fh:
            pickle.dump(bad, fh)
    finally:
        del sys.modules[mod.__name__]
    with pytest.raises(TypeError, match="convert the model file to plain numpy arrays"):
        SMPL(str(tmp_path / "wrapped"))


class _Sparse:
    """A stand-in with the two members of a scipy sparse matrix the loader looks at."""
    def __init__(self, dense):
        self.dense, self.nnz = dense, int((dense != 0).sum())

    def toarray(self):
        return self.dense


def test_sparse_joint_regressor_is_densified(model):
    from selfreconcode_amd.smpl_pytorch import SMPL
    m = dict(model)
    m["J_regressor"] = _Sparse(np.ascontiguousarray(model["J_regressor"].T))            # joints x vertices, as the official files have it
    assert torch.equal(SMPL(m).J_regressor, SMPL(model).J_regressor)


def test_getsmpl_without_a_model_directory_says_where_it_looked(tmp_path, monkeypatch):
    from selfreconcode_amd.smpl_pytorch import getSMPL
    monkeypatch.delenv("SR_SMPL_MODEL_DIR", raising=False)
    with pytest.raises(FileNotFoundError, match="SR_SMPL_MODEL_DIR"):
        getSMPL("male")
    monkeypatch.setenv("SR_SMPL_MODEL_DIR", str(tmp_path / "env"))
    with pytest.raises(FileNotFoundError) as e:
        getSMPL("female", model_dir=str(tmp_path / "arg"))
    assert str(tmp_path / "arg" / "female_smpl_with_cocoplus_reg.pkl") in str(e.value)
    assert str(tmp_path / "env" / "female_smpl_with_cocoplus_reg.txt") in str(e.value)


def test_getsmpl_finds_a_model_through_the_environment(tmp_path, monkeypatch, model):
    from selfreconcode_amd.smpl_pytorch import getSMPL
    with open(tmp_path / "neutral_smpl_with_cocoplus_reg.txt", "w") as fh:
        json.dump({k: np.asarray(v).tolist() for k, v in model.items()}, fh)
    monkeypatch.setenv("SR_SMPL_MODEL_DIR", str(tmp_path))
    smpl = getSMPL("neutral")
    assert smpl.faces == model["f"].tolist() and smpl.v_template.shape == (twin.GOLDEN_NV, 3)


def test_cpu_tensors_and_grad_inputs_are_refused(model):
    from selfreconcode_amd.smpl_pytorch import SMPL
    smpl = SMPL(model)
    beta, theta = torch.zeros(1, 10), torch.zeros(1, 24, 3)
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        smpl(beta, theta)
    with pytest.raises(RuntimeError, match="non-GPU tensor"):
        smpl.skeleton(beta)
    with pytest.raises(NotImplementedError, match="forward only"):
        smpl(beta.clone().requires_grad_(True), theta)


def test_tmp_body_normals_of_a_closed_tetrahedron():
    """The torch restatement of openmesh's vertex normals (unit face normals summed, not area weighted) needs no GPU."""
    from selfreconcode_amd.model.network import uniform_vertex_normals
    v, f, want = twin.tetrahedron_case()
    n = uniform_vertex_normals(torch.from_numpy(v).float(), torch.from_numpy(f))
    assert n.dtype == torch.float64 and not n.is_cuda and np.abs(n.numpy() - want).max() < 1e-12
    assert np.abs(twin.vertex_normals_uniform(v, f) - want).max() < 1e-12
    # area weighting would give another answer at the vertices of the slanted face
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    aw = np.zeros((4, 3))
    np.add.at(aw, f.reshape(-1), np.repeat(fn, 3, axis=0))
    assert np.abs(aw / np.linalg.norm(aw, axis=1, keepdims=True) - want).max() > 1e-2
