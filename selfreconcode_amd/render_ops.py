"""Operators of the textured renderer (csrc/texrender.hip): GPU tensors only, no autograd.  `render.py` is the public interface."""
import ctypes
from collections import namedtuple

import torch

from . import _lib
from .ops import _faces

TextureMips = namedtuple("TextureMips", "buffer R L")

MIPS_MAX_R = 32768


def mip_layout(R):
    """(sides, offsets) of the mip buffer of an R x R texture: level l + 1 has side (R_l + 1) // 2, the last level side 1; offsets are
    the levels' first texels in the concatenated buffer, in float4 units."""
    R = int(R)
    if not 1 <= R <= MIPS_MAX_R:
        raise ValueError(f"texture side must lie in [1, {MIPS_MAX_R}], got {R}")
    sides = [R]
    while sides[-1] > 1:
        sides.append((sides[-1] + 1) // 2)
    offsets = [0]
    for s in sides[:-1]:
        offsets.append(offsets[-1] + s * s)
    return sides, offsets


def _vt(vt, what):
    if vt.dim() != 2 or vt.shape[1] != 2 or vt.shape[0] == 0:
        raise ValueError(f"{what}: vt [Vt,2] expected, got {tuple(vt.shape)}")
    return _lib.f32c(vt)


def texture_mips(texture, valid=None):
    """The coverage-carrying mip pyramid of texture [R,R,3] (float32, or uint8 read as x / 255) (sr_texture_mips): premultiplied
    (rgb w, w) texels with w = 1 where `valid` [R,R] is set (None: everywhere), averaged down to 1 x 1.  -> TextureMips(buffer
    [texels,4] float32 with the levels concatenated as mip_layout(R) says, R, L)."""
    _lib.require_gpu(texture, valid)
    R = texture.shape[0]
    if tuple(texture.shape) != (R, R, 3) or (valid is not None and tuple(valid.shape) != (R, R)):
        raise ValueError(f"texture_mips: texture {tuple(texture.shape)} / valid {None if valid is None else tuple(valid.shape)}")
    sides, offsets = mip_layout(R)
    tex = texture.detach().contiguous() if texture.dtype == torch.uint8 else _lib.f32c(texture)
    ok = None if valid is None else (valid != 0).to(torch.uint8).contiguous()
    buf = torch.empty((offsets[-1] + 1, 4), dtype=torch.float32, device=tex.device)
    _lib.launch("sr_texture_mips", tex, tex, int(tex.dtype == torch.uint8), ok, R, buf)
    return TextureMips(buf, R, len(sides))


def texture_face_lod(xy_pix, faces, vt, ft, mips, bias=0.):
    """lod [N,F] float32 (sr_texture_face_lod): per image and face clamp(log2(texels per pixel) + bias, 0, L - 1) from the affine map
    pixel -> uv of the projected triangle; xy_pix [N,V,2] are `cameras.project`'s pixels.  Degenerate or out-of-range faces: L - 1."""
    _lib.require_gpu(xy_pix, faces, vt, ft, mips.buffer)
    if xy_pix.dim() != 3 or xy_pix.shape[2] != 2 or xy_pix.shape[0] == 0 or xy_pix.shape[1] == 0:
        raise ValueError(f"texture_face_lod: xy_pix [N,V,2] expected, got {tuple(xy_pix.shape)}")
    xy, faces, vt, ft = _lib.f32c(xy_pix), _faces(faces), _vt(vt, "texture_face_lod"), _faces(ft)
    if ft.shape != faces.shape or faces.shape[0] == 0:
        raise ValueError(f"texture_face_lod: ft {tuple(ft.shape)} and faces {tuple(faces.shape)} must correspond one to one")
    N, V, F = xy.shape[0], xy.shape[1], faces.shape[0]
    lod = torch.empty((N, F), dtype=torch.float32, device=xy.device)
    _lib.launch("sr_texture_face_lod", xy, xy, faces, vt, ft, N, V, F, vt.shape[0], mips.R, float(bias), mips.L, lod)
    return lod


def shade_textured(frags, ft, vt, mips, lod, background=(1., 1., 1.), hole=(.5, .5, .5), bg_image=None, return_coverage=False):
    """rgba [N,H,W,4] of the textured mesh on the fragments of `rasterize_meshes` (sr_shade_textured): a covered pixel takes the
    trilinear sample of `mips` at its interpolated uv and its face's `lod` [N,F], divided by the sampled coverage, alpha 1 (`hole`
    where the coverage is 0); an uncovered pixel takes `background`, or `bg_image` [N,H,W,3], and alpha 0.  With return_coverage:
    (rgba, coverage [N,H,W]).  No autograd; two calls give identical bits."""
    _lib.require_gpu(frags.pix_to_face, frags.bary_coords, ft, vt, mips.buffer, lod, bg_image)
    p2f = _lib.i64c(frags.pix_to_face[..., 0])
    bary = _lib.f32c(frags.bary_coords[..., 0, :])
    if p2f.dim() != 3 or 0 in p2f.shape:
        raise ValueError(f"shade_textured: pix_to_face [N,H,W,1] expected, got {tuple(frags.pix_to_face.shape)}")
    N, H, W = p2f.shape
    ft, vt = _faces(ft), _vt(vt, "shade_textured")
    F = ft.shape[0]
    if tuple(bary.shape) != (N, H, W, 3) or tuple(lod.shape) != (N, F) or F == 0:
        raise ValueError(f"shade_textured: bary_coords {tuple(frags.bary_coords.shape)} / lod {tuple(lod.shape)} for pix_to_face "
                         f"{tuple(frags.pix_to_face.shape)} and {F} faces")
    if bg_image is not None and tuple(bg_image.shape) != (N, H, W, 3):
        raise ValueError(f"shade_textured: bg_image {tuple(bg_image.shape)} for {N} images of {H} x {W}")
    if mips.buffer.shape[0] != mip_layout(mips.R)[1][-1] + 1 or mips.L != len(mip_layout(mips.R)[0]):
        raise ValueError(f"shade_textured: a mip buffer of {mips.buffer.shape[0]} texels / {mips.L} levels for R = {mips.R}")
    bg = None if bg_image is None else _lib.f32c(bg_image)
    colours = [(ctypes.c_float * 3)(*[float(c) for c in col]) for col in (background, hole)]
    dev = p2f.device
    rgba = torch.empty((N, H, W, 4), dtype=torch.float32, device=dev)
    cov = torch.empty((N, H, W), dtype=torch.float32, device=dev) if return_coverage else None
    _lib.launch("sr_shade_textured", p2f, p2f, bary, N, F, H, W, ft, vt, vt.shape[0], _lib.f32c(mips.buffer), mips.R, mips.L, _lib.f32c(lod),
                *colours, bg, rgba, cov)
    return (rgba, cov) if return_coverage else rgba
