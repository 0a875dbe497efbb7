"""What the stages after training share about a posed mesh (`OptimNetwork.render_frames` / `infer` and its previews, the texture bake, the
textured render), each written once: pose the template, rasterise it, the silhouette's mask error, float image -> bytes."""
import torch

from .ops import rasterize_meshes

FULL_RATIO = {'sdfRatio': 1., 'deformerRatio': 1., 'renderRatio': 1.}


def pose_template(net, verts, frame_ids, ratio=None):
    """The template `verts` [V,3] posed for `frame_ids` (a tensor of N ids, on the GPU) by the trained deformer, all ratios 1 unless
    `ratio` is given -> (def_verts [N,V,3] detached, defconds = [d_cond, [poses, trans]], rendcond), all of one fetch of the frames' parameters."""
    with torch.no_grad():
        poses, trans, d_cond, rendcond = [t.detach() for t in net.dataset.get_grad_parameters(frame_ids, frame_ids.device)]
    def_verts, defconds = pose_with(net, verts, poses, trans, d_cond, ratio)
    return def_verts, defconds, rendcond


def pose_with(net, verts, poses, trans, d_cond, ratio=None):
    """pose_template with the frames' parameters supplied: `verts` [V,3] posed by the trained deformer for poses [N,24,3] (or what the
    dataset's table holds per frame), trans [N,3] and the non-rigid deformer's codes d_cond [N,condlen] -- captured frames' rows or
    anything else (animate.py) -> (def_verts [N,V,3] detached, defconds = [d_cond, [poses, trans]])."""
    with torch.no_grad():
        defconds = [d_cond.detach(), [poses.detach(), trans.detach()]]
        def_verts = net.deformer(verts[None, :, :].expand(poses.shape[0], -1, 3), defconds, ratio=ratio or FULL_RATIO).detach().contiguous()
    return def_verts, defconds


def rasterize_posed(def_verts, faces, cameras, H, W, pixels=False):
    """def_verts [N,V,3] under `cameras`: project_ndc -> rasterize_meshes, and with `pixels` the vertices' pixel positions of
    cameras.project -> (frags, xy_pix [N,V,2] or None)."""
    with torch.no_grad():
        frags = rasterize_meshes(*cameras.project_ndc(def_verts), faces, H, W)
        return frags, (cameras.project(def_verts)[0] if pixels else None)


def mask_iou_error(sil, gt):
    """1 - sum(m g) / sum|m + g - m g| per frame, the reference's infer's 1 - IoU of silhouettes `sil` and masks `gt` [N,H,W] -> [N]."""
    N = sil.shape[0]
    return 1. - (sil * gt).view(N, -1).sum(1) / (sil + gt - sil * gt).abs().view(N, -1).sum(1)


def to_u8(x):
    """clamp(255 x, 0, 255) truncated to uint8, on the device `x` is on (a tensor, or a numpy array: float or bool)."""
    return torch.clamp(torch.as_tensor(x) * 255., min=0., max=255.).to(torch.uint8)
