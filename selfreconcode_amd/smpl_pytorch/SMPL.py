"""SMPL body model -- drop-in for smpl_pytorch/SMPL.py (SMPL :17-173, getSMPL :175) on the kernels of csrc/smpl.hip.

Same constructor, buffer names and shapes (`shapedirs` [nbeta, nv*3], `posedirs` [207, nv*3], `weight` [1, nv, 24] ...), the same
`forward` / `avatar` / `skeleton` signatures and the same side effects (`self.J`, `self.J_transformed`, `self.A`).  Forward only:
nothing on the training path differentiates the body model.  The body-model files are licensed and never ship here; the model is
whatever the caller supplies (a path stem as in the reference, an `.npz`, or a dict of arrays).
"""
import json
import os
import pickle

import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops

MODEL_ENTRIES = ('v_template', 'shapedirs', 'J_regressor', 'posedirs', 'kintree_table', 'cocoplus_regressor', 'weights', 'f')
MODEL_DIR_ENV = "SR_SMPL_MODEL_DIR"


def _plain_array(model, name, dtype):
    if name not in model:
        raise KeyError(f"SMPL model: entry '{name}' is missing (entries: {sorted(model)})")
    value = model[name]
    if name == 'J_regressor' and hasattr(value, 'toarray') and hasattr(value, 'nnz'):        # a scipy sparse matrix: densified
        value = value.toarray()
    if torch.is_tensor(value):
        value = value.detach().cpu().numpy()
    try:
        arr = np.asarray(value)
    except Exception as e:                                                                    # noqa: BLE001
        raise TypeError(f"SMPL model: entry '{name}' is not a plain array ({type(value).__name__})") from e
    if arr.dtype == object or arr.dtype.kind not in "fiub":
        raise TypeError(f"SMPL model: entry '{name}' is not a plain array ({type(value).__name__}, dtype {arr.dtype}); convert the model "
                        "file to plain numpy arrays first")
    return np.ascontiguousarray(arr.astype(dtype))


def load_model(model):
    """dict of the eight model entries from: a dict of arrays, a path to an `.npz`, or a path stem tried as `<stem>.pkl` then
    `<stem>.txt` (JSON), as the reference does."""
    if isinstance(model, dict):
        return model
    path = os.fspath(model)
    if path.endswith('.npz'):
        with np.load(path, allow_pickle=False) as data:
            return {k: data[k] for k in data.files}
    if os.path.isfile(path + '.pkl'):
        try:
            with open(path + '.pkl', 'rb') as reader:
                return pickle.load(reader, encoding='latin1')
        except (ImportError, AttributeError, pickle.UnpicklingError) as e:
            # an entry saved through an array wrapper (the official files use one) cannot even be unpickled without that package
            raise TypeError(f"SMPL model: {path}.pkl holds entries that are not plain arrays and cannot be unpickled here ({type(e).__name__}: {e}); "
                            "convert the model file to plain numpy arrays first") from e
    if os.path.isfile(path + '.txt'):
        with open(path + '.txt', 'r') as reader:
            return json.load(reader)
    raise FileNotFoundError(f"SMPL model: neither {path}.pkl nor {path}.txt exists")


class SMPL(nn.Module):
    def __init__(self, model, joint_type='cocoplus', obj_saveable=False):
        super().__init__()
        if joint_type not in ('cocoplus', 'lsp'):
            raise ValueError(f"SMPL: joint_type = {joint_type!r}; the regressed joints come as 'cocoplus' (19) or 'lsp' (the first 14)")
        self.model_path = model if isinstance(model, (str, os.PathLike)) else None
        self.joint_type = joint_type
        model = load_model(model)
        faces = _plain_array(model, 'f', np.int64)
        self.faces = faces.tolist() if obj_saveable else None
        self.register_buffer('faces_tensor', torch.from_numpy(faces), persistent=False)

        v_template = _plain_array(model, 'v_template', np.float64)
        nv = v_template.shape[0]
        self.size = [nv, 3]
        self.register_buffer('v_template', torch.from_numpy(v_template).float())
        shapedirs = _plain_array(model, 'shapedirs', np.float64)
        self.num_betas = shapedirs.shape[-1]
        self.register_buffer('shapedirs', torch.from_numpy(np.ascontiguousarray(shapedirs.reshape(-1, self.num_betas).T)).float())
        J_regressor = _plain_array(model, 'J_regressor', np.float64)
        if J_regressor.shape == (24, nv) and nv != 24:                       # the official files store it joints x vertices
            J_regressor = np.ascontiguousarray(J_regressor.T)
        self.register_buffer('J_regressor', torch.from_numpy(J_regressor).float())
        posedirs = _plain_array(model, 'posedirs', np.float64)
        self.register_buffer('posedirs', torch.from_numpy(np.ascontiguousarray(posedirs.reshape(-1, posedirs.shape[-1]).T)).float())
        self.parents = _plain_array(model, 'kintree_table', np.int64)[0].astype(np.int32)
        joint_regressor = _plain_array(model, 'cocoplus_regressor', np.float64)
        if joint_type == 'lsp':
            joint_regressor = np.ascontiguousarray(joint_regressor[:, :14])
        self.register_buffer('joint_regressor', torch.from_numpy(joint_regressor).float())
        weights = _plain_array(model, 'weights', np.float64)
        self.register_buffer('weight', torch.from_numpy(weights).float().reshape(-1, weights.shape[0], weights.shape[1]))
        self.register_buffer('e3', torch.eye(3).float())
        self.J = self.J_transformed = self.A = None
        for name, shape in (('shapedirs', (self.num_betas, 3 * nv)), ('J_regressor', (nv, 24)), ('posedirs', (ops.SMPL_NPOSE, 3 * nv)),
                            ('joint_regressor', (nv, self.joint_regressor.shape[1])), ('weight', (1, nv, 24))):
            if tuple(getattr(self, name).shape) != shape:
                raise ValueError(f"SMPL model: {name} has shape {tuple(getattr(self, name).shape)}, expected {shape} for {nv} vertices")
        if len(self.parents) != 24 or any(not 0 <= int(p) < i for i, p in enumerate(self.parents) if i > 0):
            raise ValueError("SMPL model: kintree_table[0] must list 24 parents, each before its children")

    # ------------------------------------------------------------------ inputs
    @staticmethod
    def _input(t, what):
        if t.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError(f"SMPL: {what} requires grad, but the body model is forward only: nothing on the training path "
                                      "differentiates it (detach the input)")
        _lib.require_gpu(t)
        return t.detach().float().contiguous()

    def _shape_stage(self, beta):
        beta = self._input(beta, "beta").view(-1, self.num_betas)
        v_shaped = ops.smpl_shape(self.v_template, self.shapedirs, beta)
        return beta, v_shaped, ops.smpl_regress(v_shaped, self.J_regressor)

    def _pose_stage(self, theta, J, theta_in_rodrigues):
        theta = self._input(theta, "theta")
        if theta_in_rodrigues:
            return ops.smpl_pose(J, self.parents, theta=theta.view(-1, 24, 3))
        return ops.smpl_pose(J, self.parents, Rs=theta.view(-1, 24, 3, 3))

    # ------------------------------------------------------------------ the reference's three entry points
    def forward(self, beta, theta, get_skin=False, theta_in_rodrigues=True):
        """joints [B,K,3] (K = 19, or 14 for 'lsp'); with get_skin (verts [B,nv,3], joints, Rs [B,24,3,3])."""
        beta, v_shaped, self.J = self._shape_stage(beta)
        Rs, feature, self.J_transformed, self.A = self._pose_stage(theta, self.J, theta_in_rodrigues)
        verts = ops.smpl_skin(v_shaped, self.weight[0], self.A, self.posedirs, feature)
        joints = ops.smpl_regress(verts, self.joint_regressor)
        if get_skin:
            return verts, joints, Rs
        return joints

    def avatar(self, Tvs, beta, theta, theta_in_rodrigues=True):
        """verts [B,nv,3]: the rest vertices Tvs [nv,3] skinned with the chain of (beta, theta); sets J_transformed only."""
        Tvs = self._input(Tvs, "Tvs")
        _, _, J = self._shape_stage(beta)
        _, _, self.J_transformed, A = self._pose_stage(theta, J, theta_in_rodrigues)
        return ops.smpl_skin(Tvs.view(-1, 3), self.weight[0], A)

    def skeleton(self, beta, require_body=False):
        _, v_shaped, J = self._shape_stage(beta)
        if require_body:
            return J, v_shaped
        return J


def getSMPL(gender, model_dir=None):
    """The model `<gender>_smpl_with_cocoplus_reg` (.pkl or .txt) from `model_dir`, then from the directory named by SR_SMPL_MODEL_DIR."""
    stem = '%s_smpl_with_cocoplus_reg' % gender
    looked = []
    for where in (model_dir, os.environ.get(MODEL_DIR_ENV)):
        if not where:
            continue
        path = os.path.join(os.fspath(where), stem)
        looked.append(path + '.pkl'); looked.append(path + '.txt')
        if os.path.isfile(path + '.pkl') or os.path.isfile(path + '.txt'):
            return SMPL(path, obj_saveable=True)
    raise FileNotFoundError(f"getSMPL: no body model {stem}.pkl / .txt for gender '{gender}': looked for {looked if looked else 'nothing'} "
                            f"(model_dir = {model_dir!r}, {MODEL_DIR_ENV} = {os.environ.get(MODEL_DIR_ENV)!r}).  The SMPL files are licensed "
                            "separately and do not ship with this package")
