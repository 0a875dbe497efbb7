"""Texture baking: the third stage of the reference pipeline (train, infer, texture) -- texture_mesh_prepare.py +
texture_mesh_extract.py -- for a UV-mapped template, on the GPU.

    python -m selfreconcode_amd.texture --gpu-ids 0 --rec-root <capture folder>/result [--num 120] [--faces 20000] [--resolution 1680] [--padding 2]
        [--placement {mean,quadric}] [--simplify {cluster,collapse}] [--simplify-report]

The reference's scripts hand the unwrap and the per-view partial textures to opendr and VideoAvatar's Isomapper and the final fill to
cv2; none of them is part of the reference repository.  What the script computes with them is restated here (restated,
unpinned):

  1. frames      fids = ceil(arange(num) frame_num / num); per frame the posed vertices deformer(verts, [d_cond, [poses, trans]]).
  2. texel map   texel (r, c), centre u = (c + 0.5) / R, v = 1 - (r + 0.5) / R, belongs to the lowest-indexed UV triangle containing it.
  3. visible[f]  the face owns a pixel of the rasterised posed mesh and its three vertices round onto set mask pixels.
  4. alpha[v]    max(0, dot(normalize(p_v - cam_pos), -n_v)).
  5. per texel   cosv = UV-barycentric blend of alpha (0 on a hidden face); colour = bilinear sample of the image at the (affine) blend
                 of the vertices' pixel positions.
  6. slots       agg_num per texel, starting at cos(normal_ang); cosv > min(slots): the first slot holding the minimum takes the view.
  7. resolve     count, mask_final = count >= check_num, view_id of the best slot, tex_median = per-channel median of the filled slots.
  8. fill        push-pull into dilate(tex_mask, int(0.1 R)) - mask_final.  The reference inpaints that region with cv2.INPAINT_TELEA;
                 this is a different, documented algorithm (texture_ops.fill), not Telea's pixels.

Files written by `export_texture`, as texture_mesh_extract.py names them: tex_mask.png, mask_final.png, tex_median.png, texture.png
(uint8(x 255)), view_id.npy and tex_predata.npz (vt, ft, tmpvs, fs, defVs, fids; the opendr camera entries are not written).

The reference leaves simplifying and unwrapping the marching-cubes template to the user, who saves the result as template/uvmap.obj.
The command honours such a file; without one it makes it (mesh_prep.prepare_template: vertex clustering to `--faces` faces and a
box-projection chart atlas), so a trained folder gives template/texture.png with no hand-made file.  Everything it
writes goes under rec_root/template/.  `--placement quadric` puts the simplified vertices at the quadric optima of their cells instead
of the cell means; `--simplify collapse` decimates by edge collapse instead of clustering (mesh_prep.simplify_collapse: a manifold
template stays one); `--simplify-report` also writes template/simplify.json (the counts of the simplification and its distance to the
extracted template).
"""
import argparse
import os
from collections import namedtuple

import numpy as np
import torch

from .infer_export import write_png
from .mesh_io import read_obj_uv
from .ops import vertex_adjacency, vertex_normals
from .posed import pose_template, rasterize_posed, to_u8
from .texture_ops import TextureAccumulator, face_visibility, fill, uv_texel_map, view_alpha

BakedTexture = namedtuple("BakedTexture", "tex_mask mask_final count view_id tex_median texture fids def_verts")


def texture_frames(frame_num, num=120):
    """The frame ids texture_mesh_prepare.py:81 bakes from: `num` ids spread over `frame_num` frames."""
    return np.ceil(np.arange(int(num)) * int(frame_num) * 1. / int(num)).astype(np.int64)


def _bake_batch(net, acc, adj, verts, faces, ratio, batch):
    device = verts.device
    fids = torch.tensor([int(b[0]) for b in batch], dtype=torch.long, device=device)
    images = torch.stack([torch.as_tensor(b[1]).to(device=device, dtype=torch.float32) for b in batch])
    masks = torch.stack([torch.as_tensor(b[2]).to(device) != 0 for b in batch])
    N = fids.numel()
    cameras, H, W = net._cameras(N, device)
    if tuple(images.shape) != (N, H, W, 3) or tuple(masks.shape) != (N, H, W):
        raise ValueError(f"bake_texture: images {tuple(images.shape)} / masks {tuple(masks.shape)} for the dataset's {H} x {W} camera")
    defV = pose_template(net, verts, fids, ratio)[0]
    frags, xy_pix = rasterize_posed(defV, faces, cameras, H, W, pixels=True)
    with torch.no_grad():
        alpha = view_alpha(defV, vertex_normals(defV, faces, adj), cameras.cam_pos().detach())
        visible = face_visibility(frags.pix_to_face[..., 0], faces, xy_pix, masks)
        acc.accumulate(fids, visible, alpha, xy_pix, images)
    return defV


def bake_texture(net, verts, faces, vt, ft, views, ratio=None, resolution=1680, agg_num=50, normal_ang=68., check_num=5, batch=8):
    """Bakes the texture of the UV-mapped template (verts [V,3], faces [F,3], vt [Vt,2], ft [F,3]; GPU tensors) from `views`, an iterable
    of (frame_id, image [H,W,3] float in [0,1], mask [H,W] bool) in frame order -- the channel order of the images is carried through
    untouched.  Each view poses the template with the trained deformer (all ratios 1 unless `ratio` is given), rasterises it under the
    dataset's camera and feeds the accumulator; `batch` views share one set of launches.  Returns BakedTexture of numpy arrays: tex_mask,
    mask_final [R,R] bool, count, view_id [R,R] int32, tex_median, texture [R,R,3] float32, fids [K], def_verts [K,V,3]."""
    from . import _lib
    _lib.require_gpu(verts, faces, vt, ft)
    verts = verts.detach().contiguous().float()
    faces = faces.long().contiguous()
    if tuple(ft.shape) != tuple(faces.shape):
        raise ValueError(f"bake_texture: ft {tuple(ft.shape)} and faces {tuple(faces.shape)} must correspond one to one")
    tmap = uv_texel_map(vt, ft, resolution)
    acc = TextureAccumulator(tmap, faces, agg_num, normal_ang)
    adj = vertex_adjacency(faces, verts.shape[0])
    fids, defVs, pending = [], [], []
    for view in views:
        pending.append(view)
        if len(pending) == int(batch):
            defVs.append(_bake_batch(net, acc, adj, verts, faces, ratio, pending).cpu())
            fids += [int(b[0]) for b in pending]
            pending = []
    if pending:
        defVs.append(_bake_batch(net, acc, adj, verts, faces, ratio, pending).cpu())
        fids += [int(b[0]) for b in pending]
    if not fids:
        raise ValueError("bake_texture: no views")
    res = acc.resolve(check_num)
    tex_mask = tmap.face >= 0
    texture = fill(res.tex_median, res.mask_final, tex_mask)
    return BakedTexture(tex_mask.cpu().numpy(), res.mask_final.cpu().numpy(), res.count.cpu().numpy(), res.view_id.cpu().numpy(),
                        res.tex_median.cpu().numpy(), texture.cpu().numpy(), np.asarray(fids, np.int64), torch.cat(defVs).numpy())


def export_texture(net, obj_path, views, out_root, ratio=None, resolution=1680, agg_num=50, normal_ang=68., check_num=5, device=None):
    """texture_mesh_prepare.py + texture_mesh_extract.py: reads the UV-mapped template `obj_path` (template/uvmap.obj), bakes it from
    `views` (see bake_texture) and writes tex_mask.png, mask_final.png, tex_median.png, texture.png, view_id.npy and tex_predata.npz under
    `out_root`.  Returns the BakedTexture."""
    v, f, vt, ft = read_obj_uv(obj_path)
    device = device or net.dataset.device
    baked = bake_texture(net, torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), torch.from_numpy(vt).to(device),
                         torch.from_numpy(ft).to(device), views, ratio, resolution, agg_num, normal_ang, check_num)
    os.makedirs(out_root, exist_ok=True)
    for name in ("tex_mask", "mask_final", "tex_median", "texture"):                               # uint8(x 255) of the values clipped to [0, 1]
        write_png(os.path.join(out_root, name + ".png"), to_u8(getattr(baked, name)).numpy())
    np.save(os.path.join(out_root, "view_id.npy"), baked.view_id)
    np.savez(os.path.join(out_root, "tex_predata.npz"), vt=vt, ft=ft, tmpvs=v, fs=f, defVs=baked.def_verts, fids=baked.fids)
    return baked


def build_parser():
    parser = argparse.ArgumentParser(prog='python -m selfreconcode_amd.texture', description='neu video body texture')
    parser.add_argument('--gpu-ids', nargs='+', type=int, metavar='IDs', default=[0], help='gpu ids')
    parser.add_argument('--num', default=120, type=int, metavar='IDs', help='Number of used frames')
    parser.add_argument('--rec-root', default=None, metavar='M', help='data root')
    parser.add_argument('--faces', default=20000, type=int, metavar='F', help='face budget of the template when template/uvmap.obj has to be made')
    parser.add_argument('--resolution', default=1680, type=int, metavar='R', help='texture size')
    parser.add_argument('--padding', default=2, type=int, metavar='P', help='texels kept free around every chart')
    parser.add_argument('--placement', default='mean', choices=['mean', 'quadric'],
                        help='where a simplified vertex goes: the mean of its cell, or the quadric optimum of the faces that touch the cell')
    parser.add_argument('--simplify', default='cluster', choices=['cluster', 'collapse'],
                        help='how the template is brought to --faces faces: vertex clustering, or edge collapse (keeps a manifold a manifold)')
    parser.add_argument('--simplify-report', action='store_true',
                        help='write template/simplify.json: the counts of the simplification and its distance to the extracted template')
    return parser


def dataset_views(dataset, fids):
    """The views bake_texture takes, one frame at a time from dataset.batch: the image from B, G, R in [-1, 1] to R, G, B in [0, 1]."""
    for f in fids:
        b = dataset.batch([int(f)])
        yield int(f), (b['img'][0].flip(-1) + 1.) * 0.5, b['mask'][0] > 0.5


def _prepare_with_report(net, args, folder, out):
    """prepare_template on the template extracted here (the same call it would make), so that the simplified mesh can be measured
    against it: writes template/simplify.json (the report of simplify_mesh or simplify_collapse, and mesh_prep.simplify_quality) and prints
    one line."""
    import json
    from .mesh_prep import prepare_template, simplify_quality
    from .posed import FULL_RATIO
    TmpVs, Tmpfs = net.discretizeSDF(FULL_RATIO, None, 0.)
    report = {}
    prep = prepare_template(net, args.rec_root, target_faces=args.faces, resolution=args.resolution, padding=args.padding, TmpVs=TmpVs, Tmpfs=Tmpfs,
                            placement=args.placement, report=report, method=args.simplify)
    if args.simplify == 'cluster':
        report['cell'] = prep.mesh.cell
    report['quality'] = quality = simplify_quality(prep.mesh, TmpVs.detach(), Tmpfs)
    path = os.path.join(folder, 'simplify.json')
    with open(path, 'w') as fh:
        json.dump(report, fh, indent=1, sort_keys=True)
        fh.write('\n')
    if args.simplify == 'collapse':
        out('simplify: method collapse, %d rounds, %d collapses%s, %d locked vertices, %d flipped / %d zero-area faces, source -> simplified mean '
            '%.3g, volume ratio %.4f; wrote %s' % (report['rounds'], report['collapses'], ' (stalled)' if report['stalled'] else '',
                                                  report['locked_vertices'], report['flipped'], report['zero_area'],
                                                  quality['source_to_simplified']['mean'], quality['volume_ratio'], path))
        return prep
    out('simplify: placement %s, %d cells (%d clamped, %d without planes), %d flipped / %d zero-area faces, source -> simplified mean %.3g, '
        'volume ratio %.4f; wrote %s' % (report['placement'], report['cells'], report['clamped'], report['no_planes'], report['flipped'],
                                         report['zero_area'], quality['source_to_simplified']['mean'], quality['volume_ratio'], path))
    return prep


def main(argv=None, out=print, resolutions=None):
    """The texture stage on a result folder: template/uvmap.obj (used if it is there, as in the reference; made by
    mesh_prep.prepare_template otherwise), then export_texture over the frames texture_frames(frame_num, --num).  `resolutions`: the
    extraction pyramid instead of infer.py's (small scenes)."""
    from .infer import load_network
    from .mesh_prep import prepare_template
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.rec_root is None:
        parser.error('--rec-root is required')
    if args.simplify == 'collapse' and args.placement != 'mean':
        parser.error('--placement %s places the representatives of --simplify cluster; --simplify collapse has no placement' % args.placement)
    device = torch.device('cuda', args.gpu_ids[0])
    net, dataset, _ = load_network(args.rec_root, device, 1, out, resolutions)
    folder = os.path.join(args.rec_root, 'template')
    obj = os.path.join(folder, 'uvmap.obj')
    if os.path.isfile(obj):
        out('reusing ' + obj)
    else:
        if args.simplify_report:
            prep = _prepare_with_report(net, args, folder, out)
        else:
            prep = prepare_template(net, args.rec_root, target_faces=args.faces, resolution=args.resolution, padding=args.padding,
                                    placement=args.placement, method=args.simplify)
        mesh, atlas = prep.mesh, prep.atlas
        out('template: %d vertices / %d faces -> %d vertices / %d faces' % (mesh.vertex_map.shape[0], prep.source_faces, mesh.verts.shape[0],
                                                                           mesh.faces.shape[0]))
        out('atlas: %d charts, scale %.4f texels per unit, overlap_texels %d' % (atlas.labels.shape[0], atlas.scale, atlas.overlap_texels))
        if atlas.overlap_texels > 0:
            out('warning: %d texels are claimed by more than one face (a chart overlaps itself in projection); they take the colour of the '
                'lowest face' % atlas.overlap_texels)
        out('wrote ' + obj)
    fids = texture_frames(dataset.frame_num, args.num)
    baked = export_texture(net, obj, dataset_views(dataset, fids), folder, resolution=args.resolution, device=device)
    out('texture: %d of %d atlas texels in mask_final; wrote %s' % (int(baked.mask_final.sum()), int(baked.tex_mask.sum()),
                                                                  os.path.join(folder, 'texture.png')))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
