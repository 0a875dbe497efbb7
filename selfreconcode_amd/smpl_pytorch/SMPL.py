"""SMPL body model -- drop-in for smpl_pytorch/SMPL.py (SMPL :17-173, getSMPL :175) on the kernels of csrc/smpl.hip.

Same constructor, buffer names and shapes (`shapedirs` [nbeta, nv*3], `posedirs` [207, nv*3], `weight` [1, nv, 24] ...), the same
`forward` / `avatar` / `skeleton` signatures and the same side effects (`self.J`, `self.J_transformed`, `self.A`).  SMPL is forward
only: nothing on the training path differentiates the body model; DifferentiableSMPL (below, on csrc/smpl_grad.hip) is the same model
with gradients, for fitting it to observations (smpl_fit.py).  The body-model files are licensed and never ship here; the model is
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


# ---------------------------------------------------------------------- the differentiable model (csrc/smpl_grad.hip)
def _no_second_order():
    if torch.is_grad_enabled():                                                # a backward under create_graph=True
        raise NotImplementedError("DifferentiableSMPL: differentiating the body model's gradient again is not supported")


def _cot(g):
    return None if g is None else _lib.f32c(g)


def _meta(*tensors):
    return [(t.shape, t.dtype) for t in tensors]


def _like(g, meta):
    """The gradient g in the shape and dtype of the input it belongs to."""
    return None if g is None else g.view(meta[0]).to(meta[1])


def _shape_backward(smpl, gJ, g_vshaped):
    """g_beta [B,nbeta] from the cotangents of the rest joints and of v_shaped (either may be None; g_vshaped is overwritten)."""
    if gJ is not None:
        g_vshaped = ops.smpl_regress_bwd(gJ, smpl.J_regressor, out=g_vshaped)
    return ops.smpl_shape_bwd(smpl.shapedirs, g_vshaped)


class _Forward(torch.autograd.Function):
    """SMPL.forward(get_skin=True) with its adjoint: (beta, theta) -> (verts, joints, Rs)."""

    @staticmethod
    def forward(ctx, beta, theta, smpl, theta_in_rodrigues):
        b = _lib.f32c(beta).view(-1, smpl.num_betas)
        v_shaped = ops.smpl_shape(smpl.v_template, smpl.shapedirs, b)
        J = ops.smpl_regress(v_shaped, smpl.J_regressor)
        th = _lib.f32c(theta).view((-1, 24, 3) if theta_in_rodrigues else (-1, 24, 3, 3))
        Rs, feature, Jt, A = ops.smpl_pose(J, smpl.parents, **({'theta': th} if theta_in_rodrigues else {'Rs': th}))
        verts = ops.smpl_skin(v_shaped, smpl.weight[0], A, smpl.posedirs, feature)
        joints = ops.smpl_regress(verts, smpl.joint_regressor)
        smpl.J, smpl.J_transformed, smpl.A = J, Jt, A
        ctx.smpl, ctx.rodrigues, ctx.meta = smpl, theta_in_rodrigues, _meta(beta, theta)
        ctx.set_materialize_grads(False)                   # an unused output's cotangent arrives as None: its kernels do not run
        ctx.save_for_backward(th, v_shaped, J, feature, A, Rs)
        return verts, joints, (Rs if theta_in_rodrigues else Rs.clone())

    @staticmethod
    def backward(ctx, g_verts, g_joints, g_Rs):
        _no_second_order()
        smpl = ctx.smpl
        th, v_shaped, J, feature, A, Rs = ctx.saved_tensors
        gV = _cot(g_verts)
        if g_joints is not None:
            gV = ops.smpl_regress_bwd(_cot(g_joints), smpl.joint_regressor, out=None if gV is None else gV.clone())
        g_rest = gA = g_feature = None
        if gV is not None:
            g_rest, gA, g_feature = ops.smpl_skin_bwd(v_shaped, smpl.weight[0], A, gV, smpl.posedirs, feature)
        g_in, gJ = ops.smpl_pose_bwd(Rs, J, A, smpl.parents, theta=th if ctx.rodrigues else None, gA=gA, g_feature=g_feature, gRs=_cot(g_Rs))
        g_beta = _shape_backward(smpl, gJ, g_rest) if ctx.needs_input_grad[0] else None
        return _like(g_beta, ctx.meta[0]), _like(g_in, ctx.meta[1]), None, None


class _Avatar(torch.autograd.Function):
    """SMPL.avatar with its adjoint: (Tvs, beta, theta) -> verts."""

    @staticmethod
    def forward(ctx, Tvs, beta, theta, smpl, theta_in_rodrigues):
        tv = _lib.f32c(Tvs).view(-1, 3)
        b = _lib.f32c(beta).view(-1, smpl.num_betas)
        J = ops.smpl_regress(ops.smpl_shape(smpl.v_template, smpl.shapedirs, b), smpl.J_regressor)
        th = _lib.f32c(theta).view((-1, 24, 3) if theta_in_rodrigues else (-1, 24, 3, 3))
        Rs, _, Jt, A = ops.smpl_pose(J, smpl.parents, **({'theta': th} if theta_in_rodrigues else {'Rs': th}))
        smpl.J_transformed = Jt
        ctx.smpl, ctx.rodrigues, ctx.meta = smpl, theta_in_rodrigues, _meta(Tvs, beta, theta)
        ctx.save_for_backward(tv, th, J, A, Rs)
        return ops.smpl_skin(tv, smpl.weight[0], A)

    @staticmethod
    def backward(ctx, g_verts):
        _no_second_order()
        smpl = ctx.smpl
        tv, th, J, A, Rs = ctx.saved_tensors
        g_rest, gA, _ = ops.smpl_skin_bwd(tv, smpl.weight[0], A, _cot(g_verts))
        g_in, gJ = ops.smpl_pose_bwd(Rs, J, A, smpl.parents, theta=th if ctx.rodrigues else None, gA=gA)
        g_beta = _shape_backward(smpl, gJ, None) if ctx.needs_input_grad[1] else None
        return _like(g_rest.sum(0), ctx.meta[0]), _like(g_beta, ctx.meta[1]), _like(g_in, ctx.meta[2]), None, None


class _Skeleton(torch.autograd.Function):
    """SMPL.skeleton(require_body=True) with its adjoint: beta -> (J, v_shaped)."""

    @staticmethod
    def forward(ctx, beta, smpl):
        b = _lib.f32c(beta).view(-1, smpl.num_betas)
        v_shaped = ops.smpl_shape(smpl.v_template, smpl.shapedirs, b)
        ctx.smpl, ctx.meta = smpl, _meta(beta)
        ctx.set_materialize_grads(False)
        return ops.smpl_regress(v_shaped, smpl.J_regressor), v_shaped

    @staticmethod
    def backward(ctx, gJ, g_vshaped):
        _no_second_order()
        g = _cot(g_vshaped)
        return _like(_shape_backward(ctx.smpl, _cot(gJ), None if g is None else g.clone()), ctx.meta[0]), None


class DifferentiableSMPL(SMPL):
    """SMPL whose three entry points carry gradients: from verts, joints and Rs to beta and theta (axis-angle or matrices), for `avatar`
    also to Tvs; `skeleton` is differentiable in beta.  The adjoints are the kernels of csrc/smpl_grad.hip behind one autograd Function
    per entry point (first order only).  With nothing to differentiate it IS SMPL: the same kernels, the same bits.  The side effects
    (`self.J`, `self.J_transformed`, `self.A`) stay detached."""

    @staticmethod
    def _wants_grad(*tensors):
        return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)

    def forward(self, beta, theta, get_skin=False, theta_in_rodrigues=True):
        if not self._wants_grad(beta, theta):
            return super().forward(beta, theta, get_skin, theta_in_rodrigues)
        _lib.require_gpu(beta, theta)
        verts, joints, Rs = _Forward.apply(beta, theta, self, theta_in_rodrigues)
        if get_skin:
            return verts, joints, Rs
        return joints

    def avatar(self, Tvs, beta, theta, theta_in_rodrigues=True):
        if not self._wants_grad(Tvs, beta, theta):
            return super().avatar(Tvs, beta, theta, theta_in_rodrigues)
        _lib.require_gpu(Tvs, beta, theta)
        return _Avatar.apply(Tvs, beta, theta, self, theta_in_rodrigues)

    def skeleton(self, beta, require_body=False):
        if not self._wants_grad(beta):
            return super().skeleton(beta, require_body)
        _lib.require_gpu(beta)
        J, v_shaped = _Skeleton.apply(beta, self)
        if require_body:
            return J, v_shaped
        return J


def getSMPL(gender, model_dir=None, differentiable=False):
    """The model `<gender>_smpl_with_cocoplus_reg` (.pkl or .txt) from `model_dir`, then from the directory named by SR_SMPL_MODEL_DIR;
    `differentiable`: as a DifferentiableSMPL."""
    stem = '%s_smpl_with_cocoplus_reg' % gender
    looked = []
    for where in (model_dir, os.environ.get(MODEL_DIR_ENV)):
        if not where:
            continue
        path = os.path.join(os.fspath(where), stem)
        looked.append(path + '.pkl'); looked.append(path + '.txt')
        if os.path.isfile(path + '.pkl') or os.path.isfile(path + '.txt'):
            return (DifferentiableSMPL if differentiable else SMPL)(path, obj_saveable=True)
    raise FileNotFoundError(f"getSMPL: no body model {stem}.pkl / .txt for gender '{gender}': looked for {looked if looked else 'nothing'} "
                            f"(model_dir = {model_dir!r}, {MODEL_DIR_ENV} = {os.environ.get(MODEL_DIR_ENV)!r}).  The SMPL files are licensed "
                            "separately and do not ship with this package")
