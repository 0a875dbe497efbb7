"""Autograd faces of csrc/step_ops.hip: the elementwise / small-matrix blocks between the MLP evaluations of one training
step (camera projection and rays, cardinal rays, the colour / normal / eikonal / deformation-regulariser / mask-IoU
reductions, the normal equations of the implicit differentiation), each one launch for the value and one for the gradient.

The composite torch formulations these replace stay in model/optim_network.py, utils/utils.py and model/CameraMine.py (they
are the reference's own lines, cited there); `ENABLED = False` (or SR_FUSED_STEP_OPS=0) switches back to them, which is how
tests/test_step_ops_gpu.py checks every fused op in value and gradient.  First-order only: none of these outputs is
differentiated twice by the step (the second-order path runs through the MLP engine, whose inputs here are plain cotangents).
"""
import ctypes
import os

import torch
from torch.autograd import Function

from . import _lib
from ._lib import f32c, i64c

ENABLED = os.environ.get("SR_FUSED_STEP_OPS", "1") != "0"
ENABLED_CAMERA = ENABLED          # model/CameraMine.py reads this one (projection / rays), everything else reads ENABLED
MAX_FRAMES = _lib.SR_STEP_MAX_FRAMES
_SLOTS = _lib.SR_STEP_LOSS_SLOTS


def _loss_buffers(rows, dev):
    blocks = _lib.raw("sr_step_reduce_blocks")(int(rows))
    out = torch.empty((_SLOTS,), dtype=torch.float32, device=dev)
    partial = torch.empty((blocks, _SLOTS - 1), dtype=torch.float32, device=dev) if blocks > 1 else None
    return out, partial


def _param_buffers(n, dev):
    """(gparams [16], per-block partials) of the camera-parameter gradient reductions over n rows."""
    blocks = max(_lib.raw("sr_step_param_blocks")(n), 1)
    return torch.empty((16,), dtype=torch.float32, device=dev), torch.empty((blocks, 16), dtype=torch.float32, device=dev)


def _gscalar(g):
    g = g.detach()
    if g.dtype != torch.float32:
        g = g.float()
    return g.reshape(1) if g.is_contiguous() else g.contiguous().reshape(1)


# ------------------------------------------------------------------------------------------------ camera
class _CamArgs:
    """sr_camera for one (R, T, f, c, W, H): keeps the tensors it points to alive."""

    def __init__(self, R, T, f, c, W, H):
        self.keep = (f32c(R), None if T is None else f32c(T), f32c(f), f32c(c))
        a = _lib.SrCamera()
        a.R, a.T, a.f, a.c = _lib.ptr(self.keep[0]), _lib.ptr(self.keep[1]), _lib.ptr(self.keep[2]), _lib.ptr(self.keep[3])
        a.W, a.H = float(W), float(H)
        a.one_minus_inv_w, a.one_minus_inv_h = 1. - 1. / float(W), 1. - 1. / float(H)
        self.c = a

    def ref(self):
        return ctypes.byref(self.c)


def _param_grads(ctx_needs, gparams, R, T, f, c):
    gR = gparams[0:9].view(3, 3).to(R.dtype).view(R.shape) if ctx_needs[0] else None
    gT = gparams[9:12].to(T.dtype).view(T.shape) if ctx_needs[1] and T is not None else None
    gf = gparams[12:14].to(f.dtype).view(f.shape) if ctx_needs[2] else None
    gc = gparams[14:16].to(c.dtype).view(c.shape) if ctx_needs[3] else None
    return gR, gT, gf, gc


class ProjectNDC(Function):
    """model/CameraMine.py:44-70,171-262 for one camera: world points [..., 3] -> NDC xy [..., 2], view depth [...]."""

    @staticmethod
    def forward(ctx, ps, R, T, f, c, W, H):
        _lib.require_gpu(ps, R, f, c)
        p = f32c(ps).view(-1, 3)
        n = p.shape[0]
        cam = _CamArgs(R, T, f, c, W, H)
        xy = torch.empty((n, 2), dtype=torch.float32, device=p.device)
        z = torch.empty((n,), dtype=torch.float32, device=p.device)
        _lib.launch("sr_cam_project_ndc_fwd", p, p, n, cam.ref(), xy, z)
        ctx.save_for_backward(p, R, T, f, c)
        ctx.WH, ctx.pshape = (W, H), ps.shape
        ctx.set_materialize_grads(False)
        return xy.view(*ps.shape[:-1], 2), z.view(ps.shape[:-1])

    @staticmethod
    def backward(ctx, gxy, gz):
        p, R, T, f, c = ctx.saved_tensors
        if gxy is None and gz is None:
            return (None,) * 7
        n = p.shape[0]
        cam = _CamArgs(R, T, f, c, *ctx.WH)
        need_p = ctx.needs_input_grad[0]
        need_par = any(ctx.needs_input_grad[1:5])
        gps = torch.empty_like(p) if need_p else None
        gparams = partial = None
        if need_par:
            gparams, partial = _param_buffers(n, p.device)
        gxy_c = None if gxy is None else f32c(gxy).view(-1, 2)
        gz_c = None if gz is None else f32c(gz).view(-1)
        _lib.launch("sr_cam_project_ndc_bwd", p, p, n, cam.ref(), gxy_c, gz_c, gps, partial, gparams)
        gR = gT = gf = gc = None
        if need_par:
            gR, gT, gf, gc = _param_grads(ctx.needs_input_grad[1:5], gparams, R, T, f, c)
        return (None if gps is None else gps.view(ctx.pshape)), gR, gT, gf, gc, None, None


class ViewRays(Function):
    """model/CameraMine.py:129-143: pixels [P,3] = (col, row, 1) -> unit world-space rays."""

    @staticmethod
    def forward(ctx, pixels, R, f, c):
        _lib.require_gpu(pixels, R, f, c)
        px = f32c(pixels).view(-1, 3)
        n = px.shape[0]
        cam = _CamArgs(R, None, f, c, 2., 2.)
        rays = torch.empty((n, 3), dtype=torch.float32, device=px.device)
        _lib.launch("sr_cam_view_rays_fwd", px, px, n, cam.ref(), rays)
        ctx.save_for_backward(px, R, f, c)
        ctx.set_materialize_grads(False)
        return rays

    @staticmethod
    def backward(ctx, grays):
        px, R, f, c = ctx.saved_tensors
        if grays is None or not any(ctx.needs_input_grad[1:]):
            return None, None, None, None
        n = px.shape[0]
        cam = _CamArgs(R, None, f, c, 2., 2.)
        gparams, partial = _param_buffers(n, px.device)
        _lib.launch("sr_cam_view_rays_bwd", px, px, n, cam.ref(), f32c(grays), partial, gparams)
        needs = (ctx.needs_input_grad[1], False, ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        gR, _, gf, gc = _param_grads(needs, gparams, R, None, f, c)
        return None, gR, gf, gc


# ------------------------------------------------------------------------------------------------ cardinal rays / normals
class CardinalRays(Function):
    """utils/utils.py:155-169 after the Jacobian: normalize(J^-1 v), rays.detach() where J is singular."""

    @staticmethod
    def forward(ctx, J, v):
        _lib.require_gpu(J, v)
        Jc, vc = f32c(J).view(-1, 3, 3), f32c(v).view(-1, 3)
        n = Jc.shape[0]
        out = torch.empty((n, 3), dtype=torch.float32, device=Jc.device)
        ok = torch.empty((n,), dtype=torch.bool, device=Jc.device)
        _lib.launch("sr_cardinal_rays_fwd", Jc, Jc, vc, n, out, ok)
        ctx.save_for_backward(Jc, vc)
        ctx.mark_non_differentiable(ok)
        ctx.set_materialize_grads(False)
        return out, ok

    @staticmethod
    def backward(ctx, gout, _gok):
        Jc, vc = ctx.saved_tensors
        if gout is None:
            return None, None
        n = Jc.shape[0]
        gJ = torch.empty_like(Jc) if ctx.needs_input_grad[0] else None
        gv = torch.empty_like(vc) if ctx.needs_input_grad[1] else None
        if gJ is None and gv is None:
            return None, None
        _lib.launch("sr_cardinal_rays_bwd", Jc, Jc, vc, n, f32c(gout), gJ, gv)
        return gJ, gv


def deformed_normals(J, onx):
    """utils/utils.py:132-153 in 'test' phase (no gradient): normalize(J^-T n), J n where J is singular."""
    _lib.require_gpu(J, onx)
    Jc, oc = f32c(J).view(-1, 3, 3), f32c(onx).view(-1, 3)
    out = torch.empty_like(oc)
    _lib.launch("sr_deformed_normals", Jc, Jc, oc, Jc.shape[0], out)
    return out


# ------------------------------------------------------------------------------------------------ loss reductions
def _pixels(b, r, c, N, H, W):
    keep = (i64c(b), i64c(r), i64c(c))
    px = _lib.SrRayPixels()
    px.b, px.r, px.c = _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2])
    px.P, px.N, px.H, px.W = keep[0].shape[0], N, H, W
    return px, keep


class ColorLoss(Function):
    """model/network.py:611-618: scatter-mean over frames of |gt[b,r,c] - colour|_1, then the mean over frames."""

    @staticmethod
    def forward(ctx, colors, gt, b, r, c):
        _lib.require_gpu(colors, gt)
        col, g = f32c(colors), f32c(gt)
        N, H, W = g.shape[0], g.shape[1], g.shape[2]
        px, keep = _pixels(b, r, c, N, H, W)
        out, partial = _loss_buffers(px.P, col.device)
        _lib.launch("sr_color_loss_fwd", col, ctypes.byref(px), col, g, partial, out)
        ctx.save_for_backward(col, g, out, *keep)
        ctx.dims = (N, H, W)
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        col, g, out, b, r, c = ctx.saved_tensors
        px, _ = _pixels(b, r, c, *ctx.dims)
        gcol = torch.empty_like(col)
        _lib.launch("sr_color_loss_bwd", col, ctypes.byref(px), col, g, out, _gscalar(gloss), gcol)
        return gcol, None, None, None, None


class NormalLoss(Function):
    """model/network.py:620-639 (see sr_normal_loss_fwd in include/selfrecon_hip.h)."""

    @staticmethod
    def forward(ctx, nx_raw, J, gt_normals, R, rays, weighted, b, r, c):
        _lib.require_gpu(nx_raw, J, gt_normals, R)
        nx, Jc, g, Rc = f32c(nx_raw).view(-1, 3), f32c(J).view(-1, 3, 3), f32c(gt_normals), f32c(R).view(3, 3)
        rc = f32c(rays).view(-1, 3) if weighted else None
        N, H, W = g.shape[0], g.shape[1], g.shape[2]
        px, keep = _pixels(b, r, c, N, H, W)
        out, partial = _loss_buffers(px.P, nx.device)
        _lib.launch("sr_normal_loss_fwd", nx, ctypes.byref(px), nx, Jc, g, Rc, rc, 1 if weighted else 0, partial, out)
        ctx.save_for_backward(nx, Jc, g, Rc, out, *keep, *(() if rc is None else (rc,)))
        ctx.dims, ctx.weighted = (N, H, W), bool(weighted)
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        saved = ctx.saved_tensors
        nx, Jc, g, Rc, out, b, r, c = saved[:8]
        rc = saved[8] if ctx.weighted else None
        px, _ = _pixels(b, r, c, *ctx.dims)
        gnx = torch.empty_like(nx)
        gJ = torch.empty_like(Jc) if ctx.needs_input_grad[1] else None
        _lib.launch("sr_normal_loss_bwd", nx, ctypes.byref(px), nx, Jc, g, Rc, rc, 1 if ctx.weighted else 0, out, _gscalar(gloss), gnx, gJ)
        return gnx, gJ, None, None, None, None, None, None, None


class EikonalLoss(Function):
    """model/network.py:547-549: ((|g| - 1)^2).mean()."""

    @staticmethod
    def forward(ctx, g):
        _lib.require_gpu(g)
        gc = f32c(g).view(-1, 3)
        out, partial = _loss_buffers(gc.shape[0], gc.device)
        _lib.launch("sr_eikonal_loss_fwd", gc, gc, gc.shape[0], partial, out)
        ctx.save_for_backward(gc)
        ctx.shape = g.shape
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        gc, = ctx.saved_tensors
        gg = torch.empty_like(gc)
        _lib.launch("sr_eikonal_loss_bwd", gc, gc, gc.shape[0], _gscalar(gloss), gg)
        return gg.view(ctx.shape)


class DefReguLoss(Function):
    """model/network.py:565-582: GMRobustError(sum_k log(s_k(J))^2, c, True).mean() with the batched 3x3 SVD on device."""

    @staticmethod
    def forward(ctx, J, c):
        _lib.require_gpu(J)
        A = f32c(J).view(-1, 3, 3)
        n = A.shape[0]
        U = torch.empty_like(A); V = torch.empty_like(A)
        S = torch.empty((n, 3), dtype=torch.float32, device=A.device)
        out, partial = _loss_buffers(n, A.device)
        _lib.launch("sr_svd3x3", A, A, n, U, S, V)
        _lib.launch("sr_def_regu_loss_fwd", A, S, n, float(c), partial, out)
        ctx.save_for_backward(U, S, V)
        ctx.c, ctx.shape = float(c), J.shape
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        U, S, V = ctx.saved_tensors
        gJ = torch.empty_like(U)
        _lib.launch("sr_def_regu_loss_bwd", U, U, S, V, U.shape[0], ctx.c, _gscalar(gloss), gJ)
        return gJ.view(ctx.shape), None


class MaskIoULoss(Function):
    """model/network.py:652-654: (1 - sum(m g) / sum |m + g - m g|) per frame, mean over frames."""

    @staticmethod
    def forward(ctx, masks, gt):
        _lib.require_gpu(masks, gt)
        m, g = f32c(masks), f32c(gt)
        N = m.shape[0]
        hw = m.numel() // N
        out, partial = _loss_buffers(m.numel(), m.device)
        _lib.launch("sr_mask_iou_loss_fwd", m, m, g, N, hw, partial, out)
        ctx.save_for_backward(m, g, out)
        return out[0]

    @staticmethod
    def backward(ctx, gloss):
        m, g, out = ctx.saved_tensors
        N = m.shape[0]
        gm = torch.empty_like(m)
        _lib.launch("sr_mask_iou_loss_bwd", m, m, g, N, m.numel() // N, out, _gscalar(gloss), gm)
        return gm, None


# ------------------------------------------------------------------------------------------------ implicit differentiation
def implicit_solve(grad_f, J, v, grad_l):
    """model/network.py:702-771 (no gradient): -> cot_f [P], rhs_tail [P,3], temp [P,3], ok [P] bool."""
    _lib.require_gpu(grad_f, J, v, grad_l)
    gf, Jc, vc, gl = f32c(grad_f).view(-1, 3), f32c(J).view(-1, 3, 3), f32c(v).view(-1, 3), f32c(grad_l).view(-1, 3)
    n = gf.shape[0]
    dev = gf.device
    cot_f = torch.empty((n,), dtype=torch.float32, device=dev)
    tail = torch.empty((n, 3), dtype=torch.float32, device=dev)
    temp = torch.empty((n, 3), dtype=torch.float32, device=dev)
    ok = torch.empty((n,), dtype=torch.bool, device=dev)
    _lib.launch("sr_implicit_solve", gf, gf, Jc, vc, gl, n, cot_f, tail, temp, ok)
    return cot_f, tail, temp, ok


def frames_supported(N):
    return ENABLED and 1 <= int(N) <= MAX_FRAMES
