"""Writing the trained avatar as a skinned glTF: the step after `animate`.

    python -m selfreconcode_amd.export_gltf --gpu-ids 0 --rec-root <capture folder>/result [--motion FILE.npz [--fps-in a] [--fps-out b]
                                            [--cond blend|nearest|frames|zero] [--cond-k K] [--cond-sigma s] [--cond-smooth f]
                                            [--trans motion|anchor]] [--influences K] [--morphs B] [--fit-frames N] [--frames N]
                                            [--batch-size B] [--out FILE.glb] [--self-check]

Training leaves a template, a non-rigid deformer with a per-frame code and a skinner whose 24 weights are looked up in a volume at the
deformed point: q_t(v) = v + offset(v, code_t), y_t(v) = sum_j w_j(q_t(v)) A_tj [q_t(v); 1] + trans_t.  A glTF skin has a rest mesh, one
fixed weight vector per vertex, inverse bind matrices, joint animation and linear morph targets.  Getting from the one to the other is
a fit over the capture's frames (skinfit_ops.py, csrc/skinfit.hip): the rest shape is the mean of q_t; per vertex the fixed weights
with at most K non-zeros that reproduce the skinner best over the fit frames; the cloth motion q_t - rest as B principal directions
(morph targets) with per-frame coefficients.  What a fixed-weight skin cannot express stays as error, and selfcheck.txt says how much.

Uses template/uvmap.obj + texture.png when the texture command has run, else the extracted template, untextured.  Plays the capture's
own frames, or a motion file as `animate` plans it.  Writes, and nothing else,

    rec_root/export/avatar.glb       (or --out) the binary glTF (gltf.py)
    rec_root/export/export.json      counts, K, B, lambda, kept variance, per-joint use, the objective of the fit and of the naive weights
    rec_root/export/selfcheck.txt    with --self-check: the file replayed by the specification's rules (gltf.replay_glb) against
                                     `animate`'s meshes of the same frames -- per frame the mean and the largest vertex distance for
                                     (a) naive weights (the field at the rest vertex, top K, renormalised) without morphs, (b) the
                                     fitted weights without morphs, (c) the file as written

Out of scope: dual-quaternion skinning, a glTF camera or lights, KTX textures, per-frame weights, retargeting, .fbx.
"""
import argparse
import json
import os

import numpy as np
import torch

EXPORT_DIR = 'export'
MORPH_CHUNK = 4096              # vertices of a chunk of the Gram matrix and of the basis
RANK_EPS = 1e-12                # an eigenvalue below this share of the largest spans nothing: its direction is left zero


# ---------------------------------------------------------------------------------------------------- the deformer, step by step
def evaluate_deformer(net, verts, poses, trans, codes, ratio=None):
    """posed.pose_with in its two steps -> (q [N,V,3] after the non-rigid translator, y [N,V,3] after the skinner -- pose_with's
    bits --, A [N,24,4,4] the posed transforms)."""
    from .posed import FULL_RATIO
    with torch.no_grad():
        ratio = ratio or FULL_RATIO
        translator, skinner = net.deformer.defs[0], net.deformer.defs[1]
        ps = verts[None, :, :].expand(poses.shape[0], -1, 3)
        q = translator(ps, codes.detach(), None, ratio=ratio)
        y = skinner(q, [poses.detach(), trans.detach()], None, ratio=ratio).detach().contiguous()
        A = skinner.posed_transforms(poses.detach())
    return q.detach().contiguous(), y, A.detach()


def field_weights(skinner, points):
    """The skinner's 24 weights at points [P,3] -> [P,24], read as LBSkinner._composite reads them."""
    from .MCAcc.grid_sampler_mine import GridSamplerMine3dFunction
    with torch.no_grad():
        nps = 2. * (points.reshape(-1, 3) - skinner.b_min) / (skinner.b_max - skinner.b_min) - 1.
        return GridSamplerMine3dFunction.apply(skinner.ws, nps.reshape(1, 1, 1, -1, 3)).view(24, -1).transpose(0, 1).contiguous()


def top_weights(w, K):
    """The K largest of w [V,24] (stable: a tie to the lower joint), renormalised -> (joints [V,K] int32, weights [V,K] float32 with
    unused slots joint 0, weight 0)."""
    val, idx = torch.sort(w.double(), dim=1, descending=True, stable=True)
    val, idx = val[:, :K], idx[:, :K]
    val = (val / val.sum(1, keepdim=True)).float()
    idx = torch.where(val > 0., idx, torch.zeros_like(idx))
    return idx.to(torch.int32).contiguous(), val.contiguous()


def fit_frame_ids(frame_num, fit_frames=None):
    """All frames, or `fit_frames` of them evenly strided."""
    if fit_frames is None or int(fit_frames) <= 0 or int(fit_frames) >= frame_num:
        return list(range(frame_num))
    return [(i * frame_num) // int(fit_frames) for i in range(int(fit_frames))]


def skin_residual(q, y, A, trans, joints, weights):
    """sum_t | sum_k w_k A_{t,j_k} [q_t; 1] - (y_t - trans_t) |^2 per vertex, float64: what fixed weights leave of the skinner."""
    from . import skinfit_ops as so
    D = so.residual_rows(q, y, A[:, :, :3, :].reshape(A.shape[0], 24, 12), trans, joints)
    return ((D * weights.double()[None, :, :, None]).sum(2) ** 2).sum(-1).sum(0)


def fit_skin(net, verts, frames=None, K=4, C=8, reg=1e-6, method="fused", fit_frames=None, batch_size=8, ratio=None):
    """Fixed skinning weights for the template `verts` [V,3] from the capture's frames as training left them (`frames`: ids, default
    all of them or `fit_frames` evenly strided) -> a dict: 'rest' [V,3] float32 (the mean of q_t, summed in float64 in ascending frame
    order, rounded once), 'joints' / 'weights' [V,K], 'objective', 'mask', 'lambda' (skinfit_ops.solve), 'cands', 'xbar', 'H',
    'frames', 'q' [T,V,3] (for fit_morphs), 'naive_joints' / 'naive_weights' (the field at the rest vertex, top K, renormalised) and
    'residual' / 'naive_residual' [V] (skin_residual of both over the fit frames)."""
    from . import skinfit_ops as so
    from .animate import training_tables
    poses, trans, codes = training_tables(net)
    ids = fit_frame_ids(poses.shape[0], fit_frames) if frames is None else [int(f) for f in frames]
    if not ids:
        raise ValueError("fit_skin: no frames")
    dev, V, T = verts.device, verts.shape[0], len(ids)
    skinner = net.deformer.defs[1]
    fids = torch.tensor(ids, dtype=torch.int64, device=dev)
    rest_sum = torch.zeros((V, 3), dtype=torch.float64, device=dev)
    w_sum = torch.zeros((V, 24), dtype=torch.float64, device=dev)
    batches = []
    for k0 in range(0, T, int(batch_size)):
        sl = fids[k0:k0 + int(batch_size)]
        q, y, A = evaluate_deformer(net, verts, poses[sl], trans[sl], codes[sl], ratio)
        for i in range(q.shape[0]):                                        # ascending frame order
            rest_sum += q[i].double()
        w_sum += field_weights(skinner, q).view(q.shape[0], V, 24).double().sum(0)
        batches.append((q, y, A, trans[sl].contiguous()))
    rest = (rest_sum / T).float()
    cands, xbar = so.candidates(w_sum / T, C)
    H = so.new_normal_matrix(V, dev)
    for q, y, A, tr in batches:
        so.accumulate(H, q, y, A, tr, cands, method)
    out = so.solve(H, xbar, cands, K, reg, method)
    naive_j, naive_w = top_weights(field_weights(skinner, rest), int(K))
    residual = torch.zeros((V,), dtype=torch.float64, device=dev)
    naive_residual = torch.zeros_like(residual)
    for q, y, A, tr in batches:
        residual += skin_residual(q, y, A, tr, out['joints'], out['weights'])
        naive_residual += skin_residual(q, y, A, tr, naive_j, naive_w)
    out.update(rest=rest, cands=cands, xbar=xbar, H=H, frames=ids, q=torch.cat([b[0] for b in batches]), naive_joints=naive_j, naive_weights=naive_w,
               residual=residual, naive_residual=naive_residual)
    return out


# ---------------------------------------------------------------------------------------------------- morph targets
def _chunks(V):
    return [(v0, min(v0 + MORPH_CHUNK, V)) for v0 in range(0, V, MORPH_CHUNK)]


def morph_coefficients(q, rest, basis):
    """c [T,B] float64 = (q_t - rest) M^T for points q [T,V,3] and a basis M [B,V,3], chunked over the vertices."""
    T, V = q.shape[0], q.shape[1]
    c = torch.zeros((T, basis.shape[0]), dtype=torch.float64, device=q.device)
    for v0, v1 in _chunks(V):
        d = (q[:, v0:v1].double() - rest[None, v0:v1].double()).reshape(T, -1)
        c += d @ basis[:, v0:v1].double().reshape(basis.shape[0], (v1 - v0) * 3).t()
    return c


def fit_morphs(q, rest, B):
    """The residual D [T, 3V] = q_t - rest as B principal directions -> {'basis' M [B,V,3] float64 (rows of unit norm, the entry of
    largest magnitude positive; a direction the data does not span is zero), 'coeffs' c = D M^T [T,B] float64, 'kept' the share of
    |D|^2 the basis keeps (1 for D = 0), 'energy' |D|^2, 'eigenvalues' [B]}.  The Gram matrix D D^T in float64, chunked over the vertices; its
    eigenvectors on the host with numpy.  Any device."""
    T, V = q.shape[0], q.shape[1]
    B = int(B)
    if B < 0:
        raise ValueError(f"fit_morphs: B >= 0 expected, got {B}")
    gram = torch.zeros((T, T), dtype=torch.float64, device=q.device)
    for v0, v1 in _chunks(V):
        d = (q[:, v0:v1].double() - rest[None, v0:v1].double()).reshape(T, -1)
        gram += d @ d.t()
    values, vectors = np.linalg.eigh(gram.cpu().numpy())
    order = np.argsort(-values, kind='stable')[:B]
    top = np.zeros((B,))
    top[:len(order)] = np.maximum(values[order], 0.)
    U = np.zeros((T, B))
    U[:, :len(order)] = vectors[:, order]
    spans = top > RANK_EPS * max(float(values.max()), 0.)
    scale = torch.from_numpy(np.where(spans, 1. / np.sqrt(np.where(spans, top, 1.)), 0.)).to(q.device)
    Ut = torch.from_numpy(U).to(q.device).t() * scale[:, None]                                   # [B,T]
    basis = torch.zeros((B, V, 3), dtype=torch.float64, device=q.device)
    for v0, v1 in _chunks(V):
        d = (q[:, v0:v1].double() - rest[None, v0:v1].double()).reshape(T, -1)
        basis[:, v0:v1] = (Ut @ d).reshape(B, v1 - v0, 3)
    flat = basis.reshape(B, V * 3)
    norm = flat.norm(dim=1, keepdim=True)
    flat = torch.where(norm > 0., flat / torch.where(norm > 0., norm, torch.ones_like(norm)), flat)
    if flat.shape[1]:
        lead = torch.gather(flat, 1, flat.abs().argmax(1, keepdim=True))
        flat = torch.where(lead < 0., -flat, flat)
    basis = flat.reshape(B, V, 3).contiguous()
    coeffs = morph_coefficients(q, rest, basis)
    total = float(torch.diagonal(gram).sum())
    kept = float((coeffs ** 2).sum()) / total if total > 0. else 1.
    return {'basis': basis, 'coeffs': coeffs, 'kept': kept, 'energy': total, 'eigenvalues': top}


# ---------------------------------------------------------------------------------------------------- the file
def _clip(net, verts, rest, basis, poses, trans, codes, batch_size, ratio=None):
    """(posed [T,V,3] as `animate` poses them, morph coefficients [T,B] float64) of a clip, in batches."""
    posed, coeffs = [], []
    for k0 in range(0, poses.shape[0], int(batch_size)):
        sl = slice(k0, k0 + int(batch_size))
        q, y, _ = evaluate_deformer(net, verts, poses[sl], trans[sl], codes[sl], ratio)
        posed.append(y)
        coeffs.append(morph_coefficients(q, rest, basis))
    return torch.cat(posed), torch.cat(coeffs)


def _distance_rows(replayed, want):
    dist = np.linalg.norm(replayed - want, axis=-1)
    return dist.mean(1), dist.max(1)


def write_selfcheck(path, rows):
    """selfcheck.txt in write_errors' layout: rows [T,6] = the mean and the largest vertex distance per frame of (a) naive weights
    without morphs, (b) fitted weights without morphs, (c) the file as written; then mean / max / min and the ten worst frames of
    each case's mean distance."""
    rows = np.asarray(rows, np.float64)
    with open(path, 'w') as fh:
        fh.write("      naive mean  naive max  fitted mean  fitted max  written mean  written max\n")
        for k, r in enumerate(rows):
            fh.write("%4d: %.6f %.6f %.6f %.6f %.6f %.6f\n" % ((k,) + tuple(r)))
        for name, col in (("naive", rows[:, 0]), ("fitted", rows[:, 2]), ("written", rows[:, 4])):
            fh.write("%s mean: %.6f, max: %.6f, min: %.6f, maxinds:" % (name, col.mean(), col.max(), col.min()))
            fh.write("".join("%d " % i for i in (-col).argsort(kind='stable')[:10]) + "\n")


def export_avatar(net, out_root, verts, faces, vt=None, ft=None, texture_png=None, motion=None, K=4, B=8, C=8, reg=1e-6, method="fused",
                  fit_frames=None, frames=None, fps=30., out=None, self_check=False, batch_size=8, cond='blend', cond_k=4, sigma=None,
                  smooth=0., trans=None, ratio=None):
    """Fits the skin and the morph targets of the template `verts` / `faces` (with `vt` / `ft` and `texture_png`, the PNG's bytes:
    textured) and writes out_root/export/ as the module docstring lists it (`out`: another path for the .glb).  motion=None plays the
    capture's own frames (the first `frames` of them) with their own codes; a motion (animate.read_motion's dict) is planned by
    animate.plan_motion with cond / cond_k / sigma / smooth / trans.  -> the dict export.json holds."""
    from . import gltf
    from .animate import _quaternions, plan_motion, training_tables
    from .ops import vertex_normals
    verts = verts.detach().contiguous().float()
    faces = faces.long()
    keep = (faces >= 0).all(1)                                            # (marching cubes marks a dropped triangle with a negative row)
    faces = faces[keep].contiguous()
    if ft is not None:
        ft = np.asarray(ft).reshape(-1, 3)[keep.cpu().numpy()]
    dev, V = verts.device, verts.shape[0]
    fit = fit_skin(net, verts, None, K, C, reg, method, fit_frames, batch_size, ratio)
    morph = fit_morphs(fit['q'], fit['rest'], B)
    if motion is None:
        poses, tr, codes = training_tables(net)
    else:
        poses, tr, codes, _ = plan_motion(net, motion, cond, cond_k, sigma, -1, smooth, trans)
    if frames is not None and int(frames) > 0:
        poses, tr, codes = poses[:int(frames)], tr[:int(frames)], codes[:int(frames)]
    posed, coeffs = _clip(net, verts, fit['rest'], morph['basis'], poses, tr, codes, batch_size, ratio)
    T = poses.shape[0]
    skinner = net.deformer.defs[1]
    normals = vertex_normals(fit['rest'][None], faces)[0]
    host = lambda t: t.detach().cpu().numpy()
    if vt is not None:
        origin, uv, new_faces = gltf.split_seams(host(faces), np.asarray(ft), np.asarray(vt))
        uvs = gltf.gltf_uv(uv)
    else:
        origin, uvs, new_faces = np.arange(V), None, host(faces)
    folder = os.path.join(out_root, EXPORT_DIR)
    os.makedirs(folder, exist_ok=True)
    path = out or os.path.join(folder, 'avatar.glb')
    joints, weights = host(fit['joints']), host(fit['weights'])
    gltf.write_glb(path, host(fit['rest'])[origin], new_faces, joints[origin], weights[origin], skinner.parents, host(skinner.Js), host(skinner.init_pose),
                   _quaternions(host(poses).astype(np.float64).reshape(T, 24, 3)), host(tr), fps=fps, normals=host(normals)[origin], uvs=uvs,
                   morphs=host(morph['basis'])[:, origin] if int(B) > 0 else None, morph_weights=host(coeffs) if int(B) > 0 else None,
                   texture_png=texture_png if vt is not None else None)
    used = (fit['weights'] > 0.)
    per_joint = torch.zeros((24,), dtype=torch.int64, device=dev).scatter_add(0, fit['joints'].long().reshape(-1), used.long().reshape(-1))
    lam = fit['lambda']
    record = {'vertices': V, 'file_vertices': int(len(origin)), 'faces': int(faces.shape[0]), 'frames': T, 'fit_frames': len(fit['frames']),
              'K': int(K), 'B': int(B), 'C': int(C), 'reg': float(reg), 'method': method, 'fps': float(fps), 'textured': vt is not None,
              'lambda': {'mean': float(lam.mean()), 'min': float(lam.min()), 'max': float(lam.max())}, 'kept_variance': morph['kept'], 'cloth_energy': morph['energy'],
              'influences_used': {str(n): int(((used.sum(1)) == n).sum()) for n in range(1, int(K) + 1)},
              'joint_use': per_joint.cpu().tolist(), 'objective_fit': float(fit['objective'].sum()),
              'residual_fit': float(fit['residual'].sum()), 'residual_naive': float(fit['naive_residual'].sum()), 'file': os.path.basename(path)}
    if self_check:
        glb = gltf.validate_glb(path)
        want = host(posed).astype(np.float64)[:, origin]
        naive = (host(fit['naive_joints'])[origin], host(fit['naive_weights'])[origin])
        rows = np.stack(_distance_rows(gltf.replay_glb(glb, morphs=False, joints_weights=naive), want)
                        + _distance_rows(gltf.replay_glb(glb, morphs=False), want) + _distance_rows(gltf.replay_glb(glb), want), 1)
        write_selfcheck(os.path.join(folder, 'selfcheck.txt'), rows)
        record['self_check'] = {'naive': float(rows[:, 0].mean()), 'fitted': float(rows[:, 2].mean()), 'written': float(rows[:, 4].mean()),
                                'written_max': float(rows[:, 5].max())}
    with open(os.path.join(folder, 'export.json'), 'w') as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    return record


# ---------------------------------------------------------------------------------------------------- the command
def build_parser():
    from .animate import CONDS
    parser = argparse.ArgumentParser(prog='python -m selfreconcode_amd.export_gltf', description='neu video body export (glTF)')
    parser.add_argument('--gpu-ids', nargs='+', type=int, metavar='IDs', default=[0], help='gpu ids')
    parser.add_argument('--batch-size', default=8, type=int, metavar='B', help='frames evaluated at once')
    parser.add_argument('--rec-root', default=None, metavar='M', help='data root')
    parser.add_argument('--motion', default=None, metavar='FILE.npz', help='play this motion instead of the capture: poses [T,24,3] or [T,72], optionally trans [T,3] and fps')
    parser.add_argument('--fps-in', default=None, type=float, metavar='a', help="the motion's frame rate (default: the file's fps, else 30)")
    parser.add_argument('--fps-out', default=None, type=float, metavar='b', help='the frame rate of the clip (default: --fps-in)')
    parser.add_argument('--cond', default='blend', choices=CONDS, help="where a motion's non-rigid code comes from")
    parser.add_argument('--cond-k', default=4, type=int, metavar='K', help='neighbours blended')
    parser.add_argument('--cond-sigma', default=None, type=float, metavar='s', help='width of the blend in pose-feature units (default: calibrated)')
    parser.add_argument('--cond-smooth', default=0., type=float, metavar='f', help='smooth the codes along time over this many frames')
    parser.add_argument('--trans', default=None, choices=('motion', 'anchor'), help="translation: the motion's, or the capture's mean")
    parser.add_argument('--influences', default=4, type=int, metavar='K', help='joints per vertex (1..8; past 4 the file has JOINTS_1 / WEIGHTS_1)')
    parser.add_argument('--morphs', default=8, type=int, metavar='B', help='morph targets (0: none)')
    parser.add_argument('--fit-frames', default=-1, type=int, metavar='N', help='fit over N evenly strided frames of the capture (all)')
    parser.add_argument('--frames', default=-1, type=int, metavar='N', help='write the first N frames only')
    parser.add_argument('--out', default=None, metavar='FILE.glb', help='where to write the file (default: export/avatar.glb)')
    parser.add_argument('--self-check', action='store_true', help='replay the file and write export/selfcheck.txt')
    return parser


def parse_args(parser, argv):
    """The arguments and the motion (read and resampled; None: the capture's own frames), or the parser's error exit."""
    from .animate import DEFAULT_FPS, read_motion, resample_motion
    args = parser.parse_args(argv)
    if args.rec_root is None:
        parser.error('--rec-root is required')
    if not 1 <= args.influences <= 8 or args.morphs < 0 or args.batch_size < 1 or not 1 <= args.cond_k <= 8:
        parser.error('--influences and --cond-k must lie in 1..8, --morphs must not be negative and --batch-size must be positive')
    if args.cond_sigma is not None and not args.cond_sigma > 0.:
        parser.error('--cond-sigma must be positive')
    for name in ('fps_in', 'fps_out'):
        if getattr(args, name) is not None and not getattr(args, name) > 0.:
            parser.error('--%s must be positive' % name.replace('_', '-'))
    motion = None
    args.fps = args.fps_out or args.fps_in or DEFAULT_FPS
    if args.motion is not None:
        try:
            motion = read_motion(args.motion)
        except (OSError, ValueError) as e:
            parser.error(str(e))
        fps_in = args.fps_in or motion['fps'] or DEFAULT_FPS
        args.fps = args.fps_out or fps_in
        if args.fps != fps_in:
            motion['poses'], motion['trans'] = resample_motion(motion['poses'], motion['trans'], fps_in, args.fps)
        motion['fps'] = args.fps
    return args, motion


def main(argv=None, out=print, resolutions=None):
    """The export stage on a result folder.  `resolutions`: the extraction pyramid load_network builds the network with instead of
    infer.py's (small scenes)."""
    from .infer import load_network
    from .posed import FULL_RATIO
    parser = build_parser()
    args, motion = parse_args(parser, argv)
    device = torch.device('cuda', args.gpu_ids[0])
    net, dataset, _ = load_network(args.rec_root, device, 1, lambda *a, **k: None, resolutions)
    if motion is not None and args.cond == 'frames' and motion['poses'].shape[0] > dataset.frame_num:
        parser.error("--cond frames: the motion has %d frames, the capture %d" % (motion['poses'].shape[0], dataset.frame_num))
    folder = os.path.join(args.rec_root, 'template')
    textured = all(os.path.isfile(os.path.join(folder, n)) for n in ('uvmap.obj', 'texture.png'))
    vt = ft = png = None
    if textured:
        from .mesh_io import read_obj_uv
        v, f, vt, ft = read_obj_uv(os.path.join(folder, 'uvmap.obj'))
        verts, faces = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
        with open(os.path.join(folder, 'texture.png'), 'rb') as fh:
            png = fh.read()
    else:
        verts, faces = net.discretizeSDF(FULL_RATIO, None, 0.)
    try:
        record = export_avatar(net, args.rec_root, verts, faces, vt, ft, png, motion, K=args.influences, B=args.morphs, fit_frames=args.fit_frames,
                               frames=args.frames, fps=args.fps, out=args.out, self_check=args.self_check, batch_size=args.batch_size,
                               cond=args.cond, cond_k=args.cond_k, sigma=args.cond_sigma, smooth=args.cond_smooth, trans=args.trans)
    except ValueError as e:
        raise SystemExit(str(e))
    check = ''
    if args.self_check:
        check = '; self check: mean distance %.6f naive, %.6f fitted, %.6f as written' % tuple(record['self_check'][k] for k in ('naive', 'fitted', 'written'))
    out('export: %d vertices (%d in the file) %s, %d frames, K %d, %d morphs keep %.4f of the cloth motion%s; wrote %s' % (
        record['vertices'], record['file_vertices'], 'textured' if textured else 'untextured', record['frames'], record['K'], record['B'],
        record['kept_variance'], check, args.out or os.path.join(args.rec_root, EXPORT_DIR, 'avatar.glb')))
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
