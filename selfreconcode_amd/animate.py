"""Playing a motion that was never filmed on the trained avatar: the step after `render`.

    python -m selfreconcode_amd.animate --gpu-ids 0 --rec-root <capture folder>/result --motion FILE.npz [--fps-in a] [--fps-out b]
                                        [--cond blend|nearest|frames|zero] [--cond-k K] [--cond-sigma s] [--cond-exclude r]
                                        [--cond-smooth f] [--trans motion|anchor] [--shaded] [--frames N] [--batch-size B]
                                        [--self-check [N]] [--video [--fps F] [--video-quality Q] [--nI]]

Training leaves a canonical template, a non-rigid deformer that takes a per-frame code, and a skinner that takes poses and a
translation.  Poses and translation come from the motion file; the code of a pose that was never filmed is blended from the codes of the
training frames whose poses are nearest in pose space (posecond_ops.py, csrc/posecond.hip).  The blend interpolates cloth codes INSIDE
the captured pose space: for a pose far from every captured one it still returns the nearest frames' codes, and conditioning.json
records how far that was (`max_d2_over_sigma2`).  Out of scope: the neural colour branch and its per-frame `rendcond` (frames are drawn
from the baked texture, or shaded), retargeting between body shapes, physics, hands.

FILE.npz holds `poses` [T,24,3] or [T,72] (axis-angle, SMPL joint order) and optionally `trans` [T,3] and `fps`; a capture folder's
smpl_rec.npz is accepted as it is.  Writes, and nothing else,

    rec_root/animation/<k>.png            frame k: the textured avatar (template/uvmap.obj + texture.png, when the texture command has run
                                          and --shaded is not given), else the extracted template Phong-shaded as infer's meshs/<fid>.png
    rec_root/animation/meshs/<k>.npy      the posed vertices [V,3] float32
    rec_root/animation/video.avi          with --video: the PNGs' pixels (video.py)
    rec_root/animation/conditioning.json  K, sigma2, per frame the neighbours, their d2 and weights, and the largest d2_0 / sigma2
    rec_root/animation/selfcheck.txt      with --self-check: captured frames re-posed with their own codes and with codes blended from
                                          the frames outside +-exclude: the silhouettes' 1 - IoU of both and the distance between them

Standard library, numpy and torch only.
"""
import argparse
import json
import math
import os
from fractions import Fraction

import numpy as np
import torch

from .posed import FULL_RATIO, mask_iou_error, pose_template, pose_with, rasterize_posed, to_u8

CALIBRATION_EXCLUDE = 15        # frames on either side that the sigma calibration leaves out: half a second at 30 fps.  A documented
#                                 default, not a tuned one: near frames share their pose AND their code, and say nothing about blending
CONDS = ('blend', 'nearest', 'frames', 'zero')
SMOOTH_RADIUS = 3.              # the Gaussian of `smooth` frames is cut at this many of them
DEFAULT_FPS = 30.


# ---------------------------------------------------------------------------------------------------- the motion file
def read_motion(path):
    """{'poses' [T,24,3] float32, 'trans' [T,3] float32 or None, 'fps' float or None} of an .npz with `poses` [T,24,3] or [T,72] and
    optionally `trans` [T,3] and `fps`.  ValueError, naming the file, for a missing `poses`, a wrong shape or a non-finite value."""
    with np.load(path) as data:
        if 'poses' not in data.files:
            raise ValueError(f"{path}: no `poses` array (found: {', '.join(sorted(data.files)) or 'nothing'})")
        poses = np.asarray(data['poses'])
        trans = np.asarray(data['trans']) if 'trans' in data.files else None
        fps = float(np.asarray(data['fps']).reshape(-1)[0]) if 'fps' in data.files else None
    if not (np.issubdtype(poses.dtype, np.floating) and ((poses.ndim == 3 and poses.shape[1:] == (24, 3)) or (poses.ndim == 2 and poses.shape[1] == 72))
            and poses.shape[0] > 0):
        raise ValueError(f"{path}: poses [T,24,3] or [T,72] floats with T > 0 expected, got {poses.dtype} {poses.shape}")
    poses = poses.reshape(-1, 24, 3).astype(np.float32)
    if trans is not None:
        if not (np.issubdtype(trans.dtype, np.floating) and trans.shape == (poses.shape[0], 3)):
            raise ValueError(f"{path}: trans [{poses.shape[0]},3] floats expected, got {trans.dtype} {trans.shape}")
        trans = trans.astype(np.float32)
    if not np.isfinite(poses).all() or (trans is not None and not np.isfinite(trans).all()):
        raise ValueError(f"{path}: non-finite values in poses or trans")
    if fps is not None and not (fps > 0. and math.isfinite(fps)):
        raise ValueError(f"{path}: fps = {fps}")
    return {'poses': poses, 'trans': trans, 'fps': fps}


def _quaternions(aa):
    """[..., 3] axis-angle -> [..., 4] unit quaternions (w, x, y, z), float64."""
    angle = np.linalg.norm(aa, axis=-1, keepdims=True)
    small = angle < 1e-12
    k = np.where(small, 0.5, np.sin(0.5 * angle) / np.where(small, 1., angle))
    return np.concatenate([np.cos(0.5 * angle), k * aa], -1)


def _axis_angles(q):
    """[..., 4] quaternions -> [..., 3] axis-angle with the angle in [0, pi], float64."""
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    q = np.where(q[..., :1] < 0., -q, q)
    s = np.linalg.norm(q[..., 1:], axis=-1, keepdims=True)
    angle = 2. * np.arctan2(s, q[..., :1])
    small = s < 1e-12
    return np.where(small, 2., angle / np.where(small, 1., s)) * q[..., 1:]


def resample_motion(poses, trans, fps_in, fps_out):
    """poses [T,24,3] and trans [T,3] (or None), float32, filmed at `fps_in` -> the same at `fps_out`: output frame k shows the time
    k / fps_out; the last one is the last whose time is not past the input's last frame.  On the host in float64: per joint the
    rotations of the two surrounding frames as unit quaternions, shortest-arc slerp (normalised lerp for dot > 1 - 1e-9), back to
    axis-angle with the angle in [0, pi]; `trans` linearly.  A time that falls exactly on an input frame copies that frame's row, so
    equal rates return the input's bits."""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 24, 3)
    T = poses.shape[0]
    if not (float(fps_in) > 0. and float(fps_out) > 0. and math.isfinite(float(fps_in)) and math.isfinite(float(fps_out))):
        raise ValueError(f"resample_motion: positive frame rates expected, got {fps_in} and {fps_out}")
    if trans is not None:
        trans = np.ascontiguousarray(trans, np.float32)
        if trans.shape != (T, 3):
            raise ValueError(f"resample_motion: trans [{T},3] expected, got {trans.shape}")
    step = Fraction(float(fps_in)) / Fraction(float(fps_out))                # input frames per output frame, exactly
    count = int((T - 1) / step) + 1
    at = [k * step for k in range(count)]
    lo = np.asarray([int(s) for s in at], np.int64)                          # (floor: s >= 0)
    w = np.asarray([float(s - int(s)) for s in at], np.float64)
    hi = np.minimum(lo + 1, T - 1)
    q0, q1 = _quaternions(poses[lo].astype(np.float64)), _quaternions(poses[hi].astype(np.float64))
    dot = (q0 * q1).sum(-1, keepdims=True)
    q1, dot = np.where(dot < 0., -q1, q1), np.abs(dot)
    ww = w[:, None, None]
    linear = dot > 1. - 1e-9
    omega = np.arccos(np.clip(dot, -1., 1.))
    so = np.where(linear, 1., np.sin(omega))
    a = np.where(linear, 1. - ww, np.sin((1. - ww) * omega) / so)
    b = np.where(linear, ww, np.sin(ww * omega) / so)
    out = _axis_angles(a * q0 + b * q1).astype(np.float32)
    exact = w == 0.
    out[exact] = poses[lo[exact]]
    out_t = None
    if trans is not None:
        out_t = ((1. - w[:, None]) * trans[lo].astype(np.float64) + w[:, None] * trans[hi].astype(np.float64)).astype(np.float32)
        out_t[exact] = trans[lo[exact]]
    return out, out_t


# ---------------------------------------------------------------------------------------------------- codes for unseen poses
def training_tables(net):
    """(poses [F,24,3], trans [F,3], codes [F,condlen]) of the capture as training left them: detached views of the dataset's tables."""
    ds = net.dataset
    F = int(ds.frame_num)
    names = list(getattr(ds, 'cond_ns', []))
    codes = ds.conds[names.index('deformer') if 'deformer' in names else 0]
    return ds.poses.detach()[:F].reshape(F, 24, 3), ds.trans.detach()[:F], codes.detach()[:F]


def smooth_codes(codes, frames):
    """codes [T,L] filtered along time with a Gaussian of standard deviation `frames`, cut at SMOOTH_RADIUS of them and renormalised
    at the edges (every output row is a convex combination of input rows)."""
    T = codes.shape[0]
    t = torch.arange(T, device=codes.device, dtype=torch.float32)
    off = t[:, None] - t[None, :]
    w = torch.exp(-0.5 * (off / float(frames)) ** 2) * (off.abs() <= SMOOTH_RADIUS * float(frames))
    return (w / w.sum(1, keepdim=True)) @ codes


def condition_codes(net, poses, K=4, sigma=None, exclude=-1, query_frames=None, smooth=0., joint_weights=None):
    """Deformer codes for `poses` [T,24,3] (GPU) from the training frames nearest in pose space -> {'codes' [T,condlen], 'idx' [T,K]
    int32, 'd2' [T,K], 'weights' [T,K], 'sigma2' float}, all tensors on the device.  `sigma` is the Gaussian's width in feature
    units; None calibrates it from the training poses (posecond_ops.calibrate_sigma2 with CALIBRATION_EXCLUDE).  `query_frames` /
    `exclude` leave the frames near each query's own out (self_check).  smooth > 0: smooth_codes, which hides the small steps a
    changing neighbour set leaves."""
    from . import posecond_ops as po
    train_poses, _, codes = training_tables(net)
    index = po.PoseIndex.build(train_poses, joint_weights)
    if sigma is None:
        sigma2 = po.calibrate_sigma2(index, CALIBRATION_EXCLUDE)
    else:
        sigma2 = float(sigma) ** 2
    idx, d2 = po.pose_neighbors(poses, index, K, query_frames, exclude)
    out, weights = po.blend_codes(idx, d2, codes, sigma2)
    if float(smooth) > 0.:
        out = smooth_codes(out, smooth)
    return {'codes': out, 'idx': idx, 'd2': d2, 'weights': weights, 'sigma2': sigma2}


def plan_motion(net, motion, cond='blend', K=4, sigma=None, exclude=-1, smooth=0., trans=None, joint_weights=None):
    """What posing `motion` (read_motion's dict, or (poses, trans)) takes -> (poses [T,24,3], trans [T,3], codes [T,condlen], info), on
    the network's device.  cond: 'blend' (condition_codes), 'nearest' (the same with K = 1: the nearest frame's code, bit for bit),
    'frames' (frame k's own code; the motion may not be longer than the capture), 'zero'.  trans: 'motion' (the file's; the default
    when it has one) or 'anchor' (the mean of the capture's translations for every frame; the default otherwise).  `info` is
    condition_codes' dict (without the codes), or None for 'frames' and 'zero'."""
    if cond not in CONDS:
        raise ValueError(f"cond must be one of {CONDS}, got {cond!r}")
    if not isinstance(motion, dict):
        motion = {'poses': motion[0], 'trans': motion[1]}
    train_poses, train_trans, train_codes = training_tables(net)
    dev = train_poses.device
    poses = torch.as_tensor(motion['poses']).to(dev).float().reshape(-1, 24, 3).contiguous()
    T = poses.shape[0]
    policy = trans or ('motion' if motion.get('trans') is not None else 'anchor')
    if policy == 'motion':
        if motion.get('trans') is None:
            raise ValueError("trans='motion': the motion has no translation (use 'anchor')")
        tr = torch.as_tensor(motion['trans']).to(dev).float().reshape(T, 3).contiguous()
    elif policy == 'anchor':
        tr = train_trans.mean(0, keepdim=True).expand(T, 3).contiguous()
    else:
        raise ValueError(f"trans must be 'motion' or 'anchor', got {trans!r}")
    info = None
    if cond == 'frames':
        if T > train_codes.shape[0]:
            raise ValueError(f"cond='frames': the motion has {T} frames, the capture {train_codes.shape[0]}")
        codes = train_codes[:T]
    elif cond == 'zero':
        codes = train_codes.new_zeros((T, train_codes.shape[1]))
    else:
        info = condition_codes(net, poses, 1 if cond == 'nearest' else K, sigma, exclude, None, smooth, joint_weights)
        codes = info.pop('codes')
    return poses, tr, codes, info


def animate(net, verts, motion, cond='blend', K=4, sigma=None, exclude=-1, smooth=0., trans=None, batch_size=8, ratio=None, joint_weights=None):
    """The template `verts` [V,3] posed for every frame of `motion` -> [T,V,3], in batches through posed.pose_with; the other
    arguments are plan_motion's."""
    poses, tr, codes, _ = plan_motion(net, motion, cond, K, sigma, exclude, smooth, trans, joint_weights)
    return torch.cat([pose_with(net, verts, poses[k:k + batch_size], tr[k:k + batch_size], codes[k:k + batch_size], ratio)[0]
                      for k in range(0, poses.shape[0], int(batch_size))])


# ---------------------------------------------------------------------------------------------------- drawing
class ShadedTemplate:
    """The extracted template drawn with the Phong preview `infer` uses for meshs/ (DESIGN.md 3.9): what stands in for a
    render.TexturedAvatar before the texture command has run.  The same `verts` and render(...)[0] as there."""

    def __init__(self, verts, faces):
        from .ops import vertex_adjacency
        self.verts, self.faces = verts.detach().contiguous().float(), faces.long().contiguous()
        self.adjacency = vertex_adjacency(self.faces, self.verts.shape[0])

    def render(self, def_verts, cameras, H, W, bg_image=None):
        from .ops import shade_phong, vertex_normals
        frags, _ = rasterize_posed(def_verts, self.faces, cameras, H, W)
        with torch.no_grad():
            rgba = shade_phong(def_verts, vertex_normals(def_verts, self.faces, self.adjacency), self.faces, frags, cameras.cam_pos().detach(), (0., 1., 0.))
            if bg_image is not None:
                bg = frags.pix_to_face[..., 0] < 0
                rgba[..., :3][bg] = bg_image[bg]
        return rgba, frags, None


def _jsonable(values):
    return [v if math.isfinite(v) else None for v in values]


def conditioning_record(cond, info, exclude, smooth):
    """What conditioning.json holds: cond, K, sigma2, exclude, smooth, per frame {'idx', 'd2', 'weights'} (null for a non-finite d2), and
    max_d2_over_sigma2 -- the largest nearest-frame distance in units of sigma2: how far the motion leaves the captured pose space."""
    record = {'cond': cond, 'K': 0, 'sigma2': None, 'exclude': int(exclude), 'smooth': float(smooth), 'frames': [], 'max_d2_over_sigma2': None}
    if info is not None:
        idx, d2, w = info['idx'].cpu().tolist(), info['d2'].cpu().tolist(), info['weights'].cpu().tolist()
        nearest = [row[0] for row in d2 if math.isfinite(row[0])]
        record.update(K=len(idx[0]), sigma2=info['sigma2'], frames=[{'idx': i, 'd2': _jsonable(d), 'weights': ww} for i, d, ww in zip(idx, d2, w)],
                      max_d2_over_sigma2=max(nearest) / info['sigma2'] if nearest else None)
    return record


def export_animation(net, motion, out_root, avatar=None, overlay=None, video=False, images=True, fps=30., quality=90, meshes=True, template=None,
                     cond='blend', K=4, sigma=None, exclude=-1, smooth=0., trans=None, batch_size=8, ratio=None, joint_weights=None):
    """Plays `motion` on the avatar under the dataset's camera and writes out_root/animation/ as the module docstring lists it.
    `avatar`: a render.TexturedAvatar; without one `template` = (verts, faces) is drawn as a ShadedTemplate.  `overlay`: an image
    [H,W,3] (RGB in [0, 1]) to draw behind the body instead of white.  video / images / fps / quality as infer_export.export_frames;
    meshes=False leaves meshs/ out.  The other arguments are plan_motion's.  -> conditioning_record's dict."""
    from .infer_export import write_png
    from .video import FrameVideo
    if avatar is None:
        if template is None:
            raise ValueError("export_animation: a TexturedAvatar or template=(verts, faces) is needed")
        avatar = ShadedTemplate(*template)
    poses, tr, codes, info = plan_motion(net, motion, cond, K, sigma, exclude, smooth, trans, joint_weights)
    device = poses.device
    folder = os.path.join(out_root, 'animation')
    os.makedirs(os.path.join(folder, 'meshs') if meshes else folder, exist_ok=True)
    film = FrameVideo(os.path.join(folder, 'video.avi'), device, fps, quality) if video else None
    try:
        for k0 in range(0, poses.shape[0], int(batch_size)):
            sl = slice(k0, k0 + int(batch_size))
            defV = pose_with(net, avatar.verts, poses[sl], tr[sl], codes[sl], ratio)[0]
            N = defV.shape[0]
            cameras, H, W = net._cameras(N, device)
            bg = None if overlay is None else torch.as_tensor(overlay).to(device).float().expand(N, H, W, 3).contiguous()
            pixels = to_u8(avatar.render(defV, cameras, H, W, bg_image=bg)[0][..., :3])
            if film is not None:
                film.add(pixels)
            pixels, defV = pixels.cpu().numpy(), defV.cpu().numpy()
            for i in range(N):
                if images:
                    write_png(os.path.join(folder, '%d.png' % (k0 + i)), pixels[i])
                if meshes:
                    np.save(os.path.join(folder, 'meshs', '%d.npy' % (k0 + i)), defV[i])
    finally:
        if film is not None:
            film.close()
    record = conditioning_record(cond, info, exclude, smooth)
    with open(os.path.join(folder, 'conditioning.json'), 'w') as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    return record


# ---------------------------------------------------------------------------------------------------- the self check
def self_check(net, verts, frames, exclude, faces=None, out_root=None, K=4, sigma=None, smooth=0., batch_size=8, ratio=None, joint_weights=None):
    """Leave-neighbours-out check of the conditioning on captured frames: each of `frames` is posed from its own pose and translation
    twice -- with its own code, and with a code blended from the training frames outside +-`exclude` of it -- and both are rasterised
    with `faces` under the dataset's camera.  -> rows [n,4] float64: the silhouettes' 1 - IoU against the frame's mask (own, blended),
    and the mean and the largest vertex distance between the two meshes.  With `out_root`, animation/selfcheck.txt in write_errors'
    layout: per frame, then mean / max / min and the ten worst of the blended silhouette and of the mean distance."""
    if faces is None:
        raise ValueError("self_check: the template's faces are needed for the silhouettes")
    frames = [int(f) for f in frames]
    if not frames or int(exclude) < 0:
        raise ValueError(f"self_check: at least one frame and exclude >= 0 expected, got {len(frames)} frames and exclude = {exclude}")
    device = verts.device
    fids = torch.tensor(frames, dtype=torch.int64, device=device)
    train_poses = training_tables(net)[0]
    blended = condition_codes(net, train_poses[fids], K, sigma, exclude, fids, smooth, joint_weights)['codes']
    rows = []
    for k0 in range(0, len(frames), int(batch_size)):
        ids = fids[k0:k0 + int(batch_size)]
        own, (_, (poses, tr)) = pose_template(net, verts, ids, ratio)[:2]
        other = pose_with(net, verts, poses, tr, blended[k0:k0 + int(batch_size)], ratio)[0]
        cameras, H, W = net._cameras(ids.numel(), device)
        gt = net.dataset.batch(ids)['mask'].float()
        err = [mask_iou_error((rasterize_posed(v, faces, cameras, H, W)[0].pix_to_face[..., 0] >= 0).float(), gt) for v in (own, other)]
        dist = (own - other).norm(dim=-1)
        rows.append(torch.stack([err[0], err[1], dist.mean(1), dist.max(1)[0]], 1).double().cpu())
    rows = torch.cat(rows).numpy()
    if out_root is not None:
        os.makedirs(os.path.join(out_root, 'animation'), exist_ok=True)
        with open(os.path.join(out_root, 'animation', 'selfcheck.txt'), 'w') as fh:
            fh.write("      mask  blended  dist mean  dist max\n")
            for f, r in zip(frames, rows):
                fh.write("%4d: %.4f %.4f %.6f %.6f\n" % ((f,) + tuple(r)))
            for name, col in (("blended mask", rows[:, 1]), ("dist mean", rows[:, 2])):
                fh.write("%s mean: %.6f, max: %.6f, min: %.6f, maxinds:" % (name, col.mean(), col.max(), col.min()))
                fh.write("".join("%d " % frames[i] for i in (-col).argsort(kind='stable')[:10]) + "\n")
    return rows


# ---------------------------------------------------------------------------------------------------- the command
def build_parser():
    from .video import add_video_arguments
    parser = argparse.ArgumentParser(prog='python -m selfreconcode_amd.animate', description='neu video body animate')
    parser.add_argument('--gpu-ids', nargs='+', type=int, metavar='IDs', default=[0], help='gpu ids')
    parser.add_argument('--batch-size', default=8, type=int, metavar='B', help='frames posed and drawn at once')
    parser.add_argument('--rec-root', default=None, metavar='M', help='data root')
    parser.add_argument('--motion', default=None, metavar='FILE.npz', help='poses [T,24,3] or [T,72], optionally trans [T,3] and fps')
    parser.add_argument('--fps-in', default=None, type=float, metavar='a', help="the motion's frame rate (default: the file's fps, else 30)")
    parser.add_argument('--fps-out', default=None, type=float, metavar='b', help='the frame rate to play at (default: --fps-in)')
    parser.add_argument('--cond', default='blend', choices=CONDS, help='where the non-rigid deformer\'s code comes from')
    parser.add_argument('--cond-k', default=4, type=int, metavar='K', help='neighbours blended')
    parser.add_argument('--cond-sigma', default=None, type=float, metavar='s', help='width of the blend in pose-feature units (default: calibrated)')
    parser.add_argument('--cond-exclude', default=-1, type=int, metavar='r', help='self check: frames on either side left out')
    parser.add_argument('--cond-smooth', default=0., type=float, metavar='f', help='smooth the codes along time over this many frames')
    parser.add_argument('--trans', default=None, choices=('motion', 'anchor'), help="translation: the motion's, or the capture's mean")
    parser.add_argument('--shaded', action='store_true', help='draw the shaded template even when a texture exists')
    parser.add_argument('--frames', default=-1, type=int, metavar='N', help='play the first N frames only')
    parser.add_argument('--nI', action='store_true', help='not save image')
    parser.add_argument('--self-check', nargs='?', const=0, default=None, type=int, metavar='N', help='also write selfcheck.txt over the first N captured frames (all)')
    add_video_arguments(parser, help='write animation/video.avi (Motion-JPEG)')
    parser.set_defaults(fps=None)
    return parser


def parse_args(parser, argv):
    """The arguments and the motion (read and resampled), or the parser's error exit."""
    from .video import check_video_arguments
    args = parser.parse_args(argv)
    if args.rec_root is None or args.motion is None:
        parser.error('--rec-root and --motion are required')
    if args.nI and not args.video:
        parser.error('--nI: without --video nothing would be drawn')
    if not 1 <= args.cond_k <= 8 or args.batch_size < 1:
        parser.error('--cond-k must lie in 1..8 and --batch-size must be positive')
    if args.cond_sigma is not None and not args.cond_sigma > 0.:
        parser.error('--cond-sigma must be positive')
    for name in ('fps_in', 'fps_out'):
        if getattr(args, name) is not None and not getattr(args, name) > 0.:
            parser.error('--%s must be positive' % name.replace('_', '-'))
    try:
        motion = read_motion(args.motion)
    except (OSError, ValueError) as e:
        parser.error(str(e))
    fps_in = args.fps_in or motion['fps'] or DEFAULT_FPS
    fps_out = args.fps_out or fps_in
    if fps_out != fps_in:
        motion['poses'], motion['trans'] = resample_motion(motion['poses'], motion['trans'], fps_in, fps_out)
    if args.frames > 0:
        motion['poses'] = motion['poses'][:args.frames]
        motion['trans'] = None if motion['trans'] is None else motion['trans'][:args.frames]
    motion['fps'] = fps_out
    if args.fps is None:
        args.fps = fps_out
    check_video_arguments(parser, args)
    return args, motion


def main(argv=None, out=print, resolutions=None):
    """The animate stage on a result folder.  `resolutions`: the extraction pyramid load_network builds the network with instead of
    infer.py's (small scenes)."""
    from .infer import load_network
    parser = build_parser()
    args, motion = parse_args(parser, argv)
    device = torch.device('cuda', args.gpu_ids[0])
    net, dataset, _ = load_network(args.rec_root, device, 1, lambda *a, **k: None, resolutions)
    T = motion['poses'].shape[0]
    if args.cond == 'frames' and T > dataset.frame_num:
        parser.error("--cond frames: the motion has %d frames, the capture %d" % (T, dataset.frame_num))
    folder = os.path.join(args.rec_root, 'template')
    textured = not args.shaded and all(os.path.isfile(os.path.join(folder, n)) for n in ('uvmap.obj', 'texture.png', 'tex_mask.png'))
    if textured:
        from .render import TexturedAvatar
        avatar = TexturedAvatar.from_folder(folder, device)
    else:
        avatar = ShadedTemplate(*net.discretizeSDF(FULL_RATIO, None, 0.))
    try:
        record = export_animation(net, motion, args.rec_root, avatar=avatar, video=args.video, images=not args.nI, fps=args.fps,
                                  quality=args.video_quality, cond=args.cond, K=args.cond_k, sigma=args.cond_sigma, smooth=args.cond_smooth,
                                  trans=args.trans, batch_size=args.batch_size)
        check = ''
        if args.self_check is not None:
            count = dataset.frame_num if args.self_check <= 0 else min(args.self_check, dataset.frame_num)
            rows = self_check(net, avatar.verts, range(count), args.cond_exclude if args.cond_exclude >= 0 else CALIBRATION_EXCLUDE,
                              faces=avatar.faces, out_root=args.rec_root, K=1 if args.cond == 'nearest' else args.cond_k, sigma=args.cond_sigma,
                              smooth=args.cond_smooth, batch_size=args.batch_size)
            check = '; self check over %d frames: mask %.4f own, %.4f blended, mean distance %.6f' % ((count,) + tuple(rows[:, :3].mean(0)))
    except ValueError as e:
        raise SystemExit(str(e))
    far = record['max_d2_over_sigma2']
    out('animation: %d frames %s, cond %s%s%s; wrote %s' % (
        T, 'textured' if textured else 'shaded', args.cond, '' if far is None else ' (K %d, sigma2 %.6g, largest d2 / sigma2 %.3g)' % (record['K'], record['sigma2'], far),
        check, os.path.join(args.rec_root, 'animation')))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
