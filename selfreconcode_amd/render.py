"""Drawing the textured avatar: the step after `texture` (train, infer, texture, render).

    python -m selfreconcode_amd.render --gpu-ids 0 --rec-root <capture folder>/result [--frames N] [--batch-size B] [--turntable K]
                                       [--turntable-frame F] [--C] [--lod-bias b] [--video [--fps F] [--video-quality Q]]

Reads rec_root/template/{uvmap.obj, texture.png, tex_mask.png} (what the texture command leaves), poses the UV-mapped template with the
trained deformer as the bake posed it, rasterises it under the dataset's camera and shades it with the mip-mapped UV shader of
csrc/texrender.hip (this package's own semantics, unpinned).  Writes

    rec_root/textured/<fid>.png    the textured body, RGB, on white -- or on the input image with --C
    rec_root/textured/errors.txt   per visited frame: mean absolute difference and PSNR against the input image (RGB in [0, 1]) over
                                   the pixels that are covered, inside the ground-truth mask and sampled with coverage >= 0.25, and the
                                   silhouette's 1 - IoU as `infer` computes it; a closing `mean:` line
    rec_root/turntable/<k>.png     with --turntable K: the posed body of one frame turned about the vertical axis through its centre
                                   by 2 pi k / K, under that frame's camera, on white (0.png is that frame's textured/<fid>.png)

    rec_root/textured/video.avi    with --video: the textured frames in the order visited, Motion-JPEG encoded on the GPU (video.py)
    rec_root/turntable/video.avi   with --video and --turntable K: the K views, one turn

and nothing outside those two folders.
"""
import argparse
import contextlib
import math
import os

import numpy as np
import torch

from .infer_export import write_png
from .mesh_io import read_obj_uv
from .posed import mask_iou_error, pose_template, rasterize_posed, to_u8
from .render_ops import shade_textured, texture_face_lod, texture_mips
from .video import FrameVideo, add_video_arguments, check_video_arguments

MIN_COVERAGE = 0.25                  # a colour divided by less atlas coverage than this is left out of the image error
PSNR_FLOOR = 1e-10                   # mean squared error floor: an exact match (or no compared pixel) reads 100 dB, not inf
TURNTABLE_BATCH = 8


class TexturedAvatar:
    """A UV-mapped template and its texture, ready to draw: verts [V,3], faces [F,3], vt [Vt,2], ft [F,3] and texture [R,R,3] (float32
    in [0, 1] or uint8) on the GPU; `valid` [R,R] marks the texels that hold colour (None: all).  The mip pyramid is built once."""

    def __init__(self, verts, faces, vt, ft, texture, valid=None):
        from . import _lib
        _lib.require_gpu(verts, faces, vt, ft, texture, valid)
        if verts.dim() != 2 or verts.shape[1] != 3:
            raise ValueError(f"TexturedAvatar: verts [V,3] expected, got {tuple(verts.shape)}")
        if faces.dim() != 2 or faces.shape[1] != 3 or tuple(ft.shape) != tuple(faces.shape):
            raise ValueError(f"TexturedAvatar: ft {tuple(ft.shape)} and faces {tuple(faces.shape)} must correspond one to one")
        self.verts = verts.detach().contiguous().float()
        self.faces, self.ft = faces.long().contiguous(), ft.long().contiguous()
        self.vt = vt.detach().contiguous().float()
        self.mips = texture_mips(texture, valid)

    @classmethod
    def from_folder(cls, template_dir, device):
        """The avatar the texture command left in `template_dir`: uvmap.obj, texture.png and tex_mask.png.  `valid` is tex_mask dilated
        as texture_ops.fill dilates it (a square window of int(0.1 R) texels, cv2.dilate's anchor): the region texture.png is filled in."""
        from PIL import Image
        v, f, vt, ft = read_obj_uv(os.path.join(template_dir, 'uvmap.obj'))
        tex = np.asarray(Image.open(os.path.join(template_dir, 'texture.png')).convert('RGB'))
        mask = np.asarray(Image.open(os.path.join(template_dir, 'tex_mask.png')).convert('L'))
        R = tex.shape[0]
        if tex.shape != (R, R, 3) or mask.shape != (R, R):
            raise ValueError(f"{template_dir}: texture.png {tex.shape} / tex_mask.png {mask.shape}: one square size expected")
        valid = _dilate_square(torch.from_numpy(mask.copy()).to(device) != 0, int(0.1 * R))
        return cls(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(vt).to(device),
                   torch.from_numpy(ft).to(device), torch.from_numpy(tex.copy()).to(device), valid)

    def render(self, def_verts, cameras, H, W, lod_bias=0., **shade_kwargs):
        """def_verts [N,V,3] (the posed template) under `cameras`: posed.rasterize_posed -> face lod -> shade_textured.
        -> (rgba [N,H,W,4], frags, coverage [N,H,W]); `shade_kwargs`: background, hole, bg_image."""
        defV = def_verts.detach().contiguous().float()
        if defV.dim() != 3 or tuple(defV.shape[1:]) != tuple(self.verts.shape):
            raise ValueError(f"render: def_verts {tuple(def_verts.shape)} for a template of {self.verts.shape[0]} vertices")
        frags, xy_pix = rasterize_posed(defV, self.faces, cameras, H, W, pixels=True)
        with torch.no_grad():
            lod = texture_face_lod(xy_pix, self.faces, self.vt, self.ft, self.mips, lod_bias)
            rgba, coverage = shade_textured(frags, self.ft, self.vt, self.mips, lod, return_coverage=True, **shade_kwargs)
        return rgba, frags, coverage


def _dilate_square(mask, k):
    """out[i, j] = any of mask over rows i - k // 2 .. i - k // 2 + k - 1 and the same columns (clipped; k <= 0: the mask itself)."""
    if k <= 0:
        return mask
    R = mask.shape[0]
    idx = torch.arange(R, device=mask.device)
    lo, hi = (idx - k // 2).clamp(0, R - 1), (idx - k // 2 + k - 1).clamp(0, R - 1)
    out = mask
    for dim in (0, 1):
        cs = torch.cumsum(out.to(torch.int64), dim)
        cs = torch.cat([torch.zeros_like(cs.narrow(dim, 0, 1)), cs], dim)
        out = (cs.index_select(dim, hi + 1) - cs.index_select(dim, lo)) > 0
    return out


def pose(net, avatar, frame_ids, ratio=None):
    """The avatar's vertices posed for `frame_ids` by the trained deformer, as the texture bake poses them (all ratios 1 unless `ratio`
    is given) -> [N,V,3]."""
    return pose_template(net, avatar.verts, torch.as_tensor(frame_ids).long().to(avatar.verts.device).reshape(-1), ratio)[0]


def turntable_vertices(def_verts, K):
    """[K,V,3]: entry 0 is def_verts [V,3] itself; entry k > 0 is c + R_y(2 pi k / K) (v - c) with c the vertex mean and
    R_y = [[cos, 0, sin], [0, 1, 0], [-sin, 0, cos]]."""
    if def_verts.dim() != 2 or def_verts.shape[1] != 3 or int(K) <= 0:
        raise ValueError(f"turntable_vertices: def_verts [V,3] and K > 0 expected, got {tuple(def_verts.shape)} and {K}")
    v = def_verts.detach()
    c = v.mean(0, keepdim=True)
    d = v - c
    out = [v]
    for k in range(1, int(K)):
        a = 2. * math.pi * k / int(K)
        cs, sn = math.cos(a), math.sin(a)
        out.append(c + torch.stack([cs * d[:, 0] + sn * d[:, 2], d[:, 1], -sn * d[:, 0] + cs * d[:, 2]], dim=1))
    return torch.stack(out)


def _film(video, path, device, fps, quality):
    return contextlib.closing(FrameVideo(path, device, fps, quality)) if video else contextlib.nullcontext()


def export_textured(net, avatar, batches, out_root, overlay=False, turntable=0, turntable_frame=None, ratio=None, lod_bias=0., video=False,
                    fps=30., quality=90):
    """Draws the avatar for `batches` -- (frame_ids, outs) as the dataloader yields them, outs['img'] [B,H,W,3] in [-1, 1] (BGR) and
    outs['mask'] [B,H,W] -- and writes textured/<fid>.png, textured/errors.txt and turntable/<k>.png (k < turntable) under `out_root`,
    as the module docstring lists them.  `turntable_frame`: the frame whose pose is turned (default: the first visited one).
    video=True adds textured/video.avi and turntable/video.avi: the PNGs' pixels, in the order written, at `fps` and JPEG `quality`.
    Returns {fid: (l1, psnr, mask error)}."""
    device = avatar.verts.device
    folder = os.path.join(out_root, 'textured')
    os.makedirs(folder, exist_ok=True)
    errors, turn = {}, None
    with _film(video, os.path.join(folder, 'video.avi'), device, fps, quality) as film:
        for frame_ids, outs in batches:
            fids = torch.as_tensor(frame_ids).long().to(device).reshape(-1)
            N = fids.numel()
            cameras, H, W = net._cameras(N, device)
            image = (outs['img'].to(device).float().flip(-1) + 1.) * 0.5                       # B, G, R in [-1, 1] -> R, G, B in [0, 1]
            gtM = outs['mask'].to(device).float()
            if tuple(image.shape) != (N, H, W, 3) or tuple(gtM.shape) != (N, H, W):
                raise ValueError(f"export_textured: images {tuple(image.shape)} / masks {tuple(gtM.shape)} for the dataset's {H} x {W} camera")
            defV = pose(net, avatar, fids, ratio)
            rgba, frags, coverage = avatar.render(defV, cameras, H, W, lod_bias=lod_bias, bg_image=image.contiguous() if overlay else None)
            rgb = rgba[..., :3]
            covered = frags.pix_to_face[..., 0] >= 0
            maskE = mask_iou_error(covered.float(), gtM)
            use = (covered & (gtM > 0.5) & (coverage >= MIN_COVERAGE)).float()[..., None]
            n = (3. * use.view(N, -1).sum(1)).clamp(min=1.)
            diff = (rgb.clamp(0., 1.) - image) * use
            l1 = diff.abs().view(N, -1).sum(1) / n
            psnr = 10. * torch.log10(1. / (diff.square().view(N, -1).sum(1) / n).clamp(min=PSNR_FLOOR))
            pixels = to_u8(rgb)
            if film is not None:
                film.add(pixels)
            pixels = pixels.cpu().numpy()
            for i, fid in enumerate(fids.tolist()):
                write_png(os.path.join(folder, '%d.png' % fid), pixels[i])
                errors[fid] = (float(l1[i]), float(psnr[i]), float(maskE[i]))
                if turn is None and (turntable_frame is None or fid == int(turntable_frame)):
                    turn = (fid, defV[i])
    if not errors:
        raise ValueError("export_textured: no frames")
    with open(os.path.join(folder, 'errors.txt'), 'w') as fh:
        fh.write("      l1     psnr   mask\n")
        for fid in sorted(errors):
            fh.write("%4d: %.4f %6.2f %.4f\n" % ((fid,) + errors[fid]))
        fh.write("mean: %.4f %6.2f %.4f\n" % tuple(np.mean(np.asarray([errors[f] for f in sorted(errors)], np.float64), axis=0)))
    if int(turntable) > 0:
        if turn is None:                                                                     # a frame outside the visited ones
            turn = (int(turntable_frame), pose(net, avatar, [int(turntable_frame)], ratio)[0])
        os.makedirs(os.path.join(out_root, 'turntable'), exist_ok=True)
        views = turntable_vertices(turn[1], int(turntable))
        with _film(video, os.path.join(out_root, 'turntable', 'video.avi'), device, fps, quality) as film:
            for k0 in range(0, int(turntable), TURNTABLE_BATCH):
                chunk = views[k0:k0 + TURNTABLE_BATCH]
                cameras, H, W = net._cameras(chunk.shape[0], device)
                rgb = avatar.render(chunk, cameras, H, W, lod_bias=lod_bias)[0][..., :3]
                pixels = to_u8(rgb)
                if film is not None:
                    film.add(pixels)
                pixels = pixels.cpu().numpy()
                for i in range(chunk.shape[0]):
                    write_png(os.path.join(out_root, 'turntable', '%d.png' % (k0 + i)), pixels[i])
    return errors


def build_parser():
    parser = argparse.ArgumentParser(prog='python -m selfreconcode_amd.render', description='neu video body textured render')
    parser.add_argument('--gpu-ids', nargs='+', type=int, metavar='IDs', default=[0], help='gpu ids')
    parser.add_argument('--batch-size', default=1, type=int, metavar='B', help='batch size')
    parser.add_argument('--rec-root', default=None, metavar='M', help='data root')
    parser.add_argument('--frames', default=-1, type=int, metavar='frames', help='render frame nums')
    parser.add_argument('--turntable', default=0, type=int, metavar='K', help='number of turntable views of one posed frame')
    parser.add_argument('--turntable-frame', default=None, type=int, metavar='F', help='the frame the turntable turns (default: the first one rendered)')
    parser.add_argument('--C', action='store_true', help='overlay on gtimg')
    parser.add_argument('--lod-bias', default=0., type=float, metavar='b', help='added to every level of detail (negative: sharper)')
    add_video_arguments(parser, help='write textured/video.avi and turntable/video.avi (Motion-JPEG)')
    return parser


def main(argv=None, out=print, resolutions=None):
    """The render stage on a result folder the texture command has run on.  `resolutions`: the extraction pyramid load_network builds
    the network with instead of infer.py's (small scenes)."""
    from .infer import limited, load_network
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.rec_root is None:
        parser.error('--rec-root is required')
    check_video_arguments(parser, args)
    folder = os.path.join(args.rec_root, 'template')
    for name in ('uvmap.obj', 'texture.png', 'tex_mask.png'):
        if not os.path.isfile(os.path.join(folder, name)):
            raise SystemExit('%s not found: run the texture command first (python -m selfreconcode_amd.texture --rec-root %s)'
                             % (os.path.join(folder, name), args.rec_root))
    device = torch.device('cuda', args.gpu_ids[0])
    net, dataset, dataloader = load_network(args.rec_root, device, args.batch_size, out, resolutions)
    if args.turntable_frame is not None and not 0 <= args.turntable_frame < dataset.frame_num:
        parser.error('--turntable-frame %d: the capture has frames 0 .. %d' % (args.turntable_frame, dataset.frame_num - 1))
    avatar = TexturedAvatar.from_folder(folder, device)
    errors = export_textured(net, avatar, limited(dataloader, args.batch_size, args.frames), args.rec_root, overlay=args.C,
                             turntable=args.turntable, turntable_frame=args.turntable_frame, lod_bias=args.lod_bias,
                             video=args.video, fps=args.fps, quality=args.video_quality)
    mean = np.mean(np.asarray(list(errors.values()), np.float64), axis=0)
    out('textured: %d frames, mean l1 %.4f, psnr %.2f, mask %.4f; wrote %s' % (len(errors), mean[0], mean[1], mean[2],
                                                                               os.path.join(args.rec_root, 'textured')))
    if args.turntable > 0:
        out('turntable: %d views; wrote %s' % (args.turntable, os.path.join(args.rec_root, 'turntable')))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
