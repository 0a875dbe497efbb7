"""Operators of the texture bake (csrc/texture.hip): GPU tensors only, no autograd.  `texture.py` is the public interface."""
import math
from collections import namedtuple

import torch

from . import _lib
from .ops import _faces, _require_square, _verts

TexelMap = namedtuple("TexelMap", "face bary texel tface tbary R")


def uv_texel_map(vt, ft, resolution):
    """Texel -> UV face map of a template, once per template (sr_uv_rasterize): face [R,R] int32 (-1: none), bary [R,R,3], and the
    compacted list of covered texels the accumulator works on -- texel [T] (index r R + c, ascending), tface [T], tbary [T,3].
    `tex_mask` is `face >= 0`.  Two calls give identical bits."""
    _lib.require_gpu(vt, ft)
    if vt.dim() != 2 or vt.shape[1] != 2:
        raise ValueError(f"vt [Vt,2] expected, got {tuple(vt.shape)}")
    vt = _lib.f32c(vt); ft = _faces(ft)
    R, dev = int(resolution), vt.device
    face = torch.empty((max(R, 0), max(R, 0)), dtype=torch.int32, device=dev)
    bary = torch.empty((max(R, 0), max(R, 0), 3), dtype=torch.float32, device=dev)
    _lib.launch("sr_uv_rasterize", vt, vt, ft, vt.shape[0], ft.shape[0], R, face, bary)
    texel = torch.nonzero(face.view(-1) >= 0).view(-1)
    return TexelMap(face, bary, texel.int(), face.view(-1)[texel].contiguous(), bary.view(-1, 3)[texel].contiguous(), R)


def face_visibility(pix_to_face, faces, xy_pix, masks):
    """visible [N,F] uint8 (sr_face_visibility): the face owns a pixel of `pix_to_face` [N,H,W] (rasterize_meshes' packed indices) and its
    three vertices' pixel positions xy_pix [N,V,2] round into the viewport onto a set pixel of masks [N,H,W]."""
    _lib.require_gpu(pix_to_face, faces, xy_pix, masks)
    p2f = _lib.i64c(pix_to_face); faces = _faces(faces)
    xy = _lib.f32c(xy_pix)
    N, H, W = p2f.shape
    _require_square(H, W, "face_visibility")
    if xy.dim() != 3 or xy.shape[0] != N or xy.shape[2] != 2 or tuple(masks.shape) != (N, H, W):
        raise ValueError(f"face_visibility: xy_pix {tuple(xy.shape)} / masks {tuple(masks.shape)} for pix_to_face {tuple(p2f.shape)}")
    m = (masks != 0).to(torch.uint8).contiguous()
    vis = torch.empty((N, faces.shape[0]), dtype=torch.uint8, device=xy.device)
    _lib.launch("sr_face_visibility", xy, p2f, faces, N, xy.shape[1], faces.shape[0], xy, m, H, W, vis)
    return vis


def view_alpha(verts, normals, cam_pos):
    """alpha [N,V] = max(0, dot(normalize(verts - cam_pos), -normals)) (sr_view_alpha); cam_pos [3] or [N,3]."""
    _lib.require_gpu(verts, normals)
    v = _verts(verts); n = _lib.f32c(normals)
    if n.shape != v.shape:
        raise ValueError(f"view_alpha: normals {tuple(n.shape)} for verts {tuple(v.shape)}")
    cam = torch.as_tensor(cam_pos, dtype=torch.float32).to(v.device).reshape(-1, 3).expand(v.shape[0], 3).contiguous()
    out = torch.empty(v.shape[:2], dtype=torch.float32, device=v.device)
    _lib.launch("sr_view_alpha", v, v, n, cam, v.shape[0], v.shape[1], out)
    return out


Resolved = namedtuple("Resolved", "count mask_final view_id tex_median")


class TextureAccumulator:
    """The agg_num best-seen candidates of every covered texel, slot-major in HBM: slot_cos / slot_view [agg_num,T], slot_rgb
    [agg_num,3,T] (view -1: empty), plus the per-texel fill count and running minimum.  `accumulate` takes any number of views, in frame
    order; K calls with one view and one call with K views leave identical bits."""

    def __init__(self, texel_map, faces, agg_num=50, normal_ang=68.):
        _lib.require_gpu(texel_map.tface, faces)
        if not 0. <= float(normal_ang) <= 90.:
            raise ValueError(f"normal_ang must lie in [0, 90] degrees, got {normal_ang}")       # (cosv0 >= 0: a hidden face, cosine 0, never enters)
        if int(agg_num) <= 0:
            raise ValueError(f"agg_num must be positive, got {agg_num}")
        self.map, self.faces, self.agg_num = texel_map, _faces(faces), int(agg_num)
        if self.faces.shape[0] != 0 and texel_map.tface.numel() and int(texel_map.tface.max()) >= self.faces.shape[0]:
            raise ValueError("texel map and faces disagree: the UV faces ft and the mesh faces must correspond one to one")
        self.cosv0 = max(float(torch.tensor(math.cos(float(normal_ang) / 180. * math.pi), dtype=torch.float32)), 0.)
        T, dev, A = texel_map.tface.shape[0], faces.device, self.agg_num
        self.T = T
        self.slot_cos = torch.full((A, T), self.cosv0, dtype=torch.float32, device=dev)
        self.slot_rgb = torch.zeros((A, 3, T), dtype=torch.float32, device=dev)
        self.slot_view = torch.full((A, T), -1, dtype=torch.int32, device=dev)
        self.count = torch.zeros((T,), dtype=torch.int32, device=dev)
        self.min_cos = torch.full((T,), self.cosv0, dtype=torch.float32, device=dev)
        self.min_idx = torch.zeros((T,), dtype=torch.int32, device=dev)

    def accumulate(self, fids, visible, alpha, xy_pix, images):
        """Steps 5-6 for views in order: fids [N] (what view_id reports), visible [N,F] uint8, alpha [N,V], xy_pix [N,V,2] (pixel
        positions, integer coordinates = pixel centres), images [N,H,W,3]."""
        _lib.require_gpu(visible, alpha, xy_pix, images)
        if images.dim() != 4 or images.shape[3] != 3:
            raise ValueError(f"images [N,H,W,3] expected, got {tuple(images.shape)}")
        N, H, W = images.shape[:3]
        _require_square(H, W, "TextureAccumulator.accumulate")
        F = self.faces.shape[0]
        V = alpha.shape[1]
        if tuple(visible.shape) != (N, F) or visible.dtype != torch.uint8 or tuple(alpha.shape) != (N, V) or tuple(xy_pix.shape) != (N, V, 2):
            raise ValueError(f"accumulate: visible {tuple(visible.shape)} {visible.dtype} / alpha {tuple(alpha.shape)} / xy_pix {tuple(xy_pix.shape)} "
                             f"for {N} views of {F} faces")
        if self.T == 0:
            return
        dev = images.device
        fid = torch.as_tensor(fids).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if fid.numel() != N:
            raise ValueError(f"accumulate: {fid.numel()} frame ids for {N} views")
        img, al, xy = _lib.f32c(images), _lib.f32c(alpha), _lib.f32c(xy_pix)
        vis = visible.contiguous()
        _lib.launch("sr_texture_accumulate", img, self.T, self.map.tface, self.map.tbary, self.faces, F, V, N, vis, al, xy, img, H, W, fid,
                    self.agg_num, self.cosv0, self.slot_cos, self.slot_rgb, self.slot_view, self.count, self.min_cos, self.min_idx)

    def resolve(self, check_num=5):
        """Step 7 on the [R,R] grid: count int32, mask_final bool, view_id int32 (-1 outside mask_final), tex_median [R,R,3] float32."""
        if int(check_num) <= 0:
            raise ValueError(f"check_num must be positive, got {check_num}")
        R, dev = self.map.R, self.slot_cos.device
        count = torch.zeros((R, R), dtype=torch.int32, device=dev)
        mask_final = torch.zeros((R, R), dtype=torch.uint8, device=dev)
        view_id = torch.full((R, R), -1, dtype=torch.int32, device=dev)
        med = torch.zeros((R, R, 3), dtype=torch.float32, device=dev)
        if self.T:
            _lib.launch("sr_texture_resolve", med, self.T, self.map.texel, self.agg_num, self.cosv0, int(check_num), self.slot_cos, self.slot_rgb,
                        self.slot_view, count, mask_final, view_id, med)
        return Resolved(count, mask_final.bool(), view_id, med)


def resolve(accumulator, check_num=5):
    return accumulator.resolve(check_num)


def fill(tex_median, mask_final, tex_mask, dilate=None):
    """Step 8: texture [R,R,3] = tex_median on mask_final (bit for bit); a push-pull fill on the square dilation of tex_mask by `dilate`
    texels (default int(0.1 R)) minus mask_final; 0 elsewhere.  Push-pull: the known texels are averaged down a 2x pyramid to 1 x 1
    (a cell is the mean of its known children), then every unknown cell takes the bilinear sample of the next coarser level.  This is
    NOT cv2.INPAINT_TELEA, which the reference uses (a sequential fast-marching front): smooth, local, but not that algorithm's pixels."""
    _lib.require_gpu(tex_median, mask_final, tex_mask)
    R = tex_median.shape[0]
    if tuple(tex_median.shape) != (R, R, 3) or tuple(mask_final.shape) != (R, R) or tuple(tex_mask.shape) != (R, R):
        raise ValueError(f"fill: tex_median {tuple(tex_median.shape)} / mask_final {tuple(mask_final.shape)} / tex_mask {tuple(tex_mask.shape)}")
    k = int(0.1 * R) if dilate is None else int(dilate)
    tex = _lib.f32c(tex_median)
    mf = (mask_final != 0).to(torch.uint8).contiguous(); tm = (tex_mask != 0).to(torch.uint8).contiguous()
    ws = _lib.workspace("sr_texture_fill_workspace_bytes", R, device=tex.device)
    out = torch.empty_like(tex)
    _lib.launch("sr_texture_fill", tex, tex, mf, tm, R, k, out, ws)
    return out
