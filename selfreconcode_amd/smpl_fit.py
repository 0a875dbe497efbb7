"""Fit the SMPL body model to 2-D keypoints of a sequence under the folder's one camera, and write the `smpl_rec.npz` the pipeline
starts from.  The staging is SMPLify's without its licensed pose prior; the semantics are this package's own:

  energy   sum_t sum_k (w_k c_tk)^2 rho_sigma(|project(J_tk + trans_t) - kp_tk|)          (ops.keypoint_energy, value + gradient in a launch)
           + l_theta sum_t |theta_t[1:]|^2 + l_beta |beta|^2 + l_s sum_t |J3d_{t+1} - J3d_t|^2 [+ l_3 sum |J3d - target|^2]
  stage 0  closed-form translation from the torso's 2-D size (numpy, initial_translation)
  stage 1  root orientation + translation on the torso joints, once from every start orientation; the start with the lower energy wins
  stage 2  all of theta, trans and the one shared beta, in rounds with falling priors

The optimiser is FusedAdam with fixed iteration counts; nothing is read back inside the loops (the energies go to a device buffer and
the winning start is selected on the device), and no random numbers are consumed: two runs give identical bits.

Keypoints come in the order of the model's regressed joints (joint_type='cocoplus'): 0-5 R ankle, R knee, R hip, L hip, L knee,
L ankle; 6-11 R wrist, R elbow, R shoulder, L shoulder, L elbow, L wrist; 12 neck, 13 head top; 14-18 nose, L eye, R eye, L ear, R ear.
convert_keypoints maps the COCO-18 and BODY-25 detector layouts onto it (HMR's convention, written down from memory: no model file
was at hand to check the tables against -- `joint_weights` lets a caller down-weight joints whose definition differs, the hips first).

With `masks` the silhouette term of DESIGN 3.21 joins in further rounds after stage 2 (silhouette_stages): l_in sum_t e_in[t] +
l_cov sum_t e_cov[t], the body's vertices against the exact distance field of the masks (distance_transform) and the masks' contour
samples against the vertices (silhouette_field, silhouette_energy; csrc/silfit.hip).
"""
import glob
import json
import os
import re
from collections import namedtuple

import numpy as np
import torch

from . import ops
from .optim import FusedAdam

NUM_KEYPOINTS = 19
R_HIP, L_HIP, R_SHOULDER, L_SHOULDER = 2, 3, 8, 9
TORSO = (R_HIP, L_HIP, R_SHOULDER, L_SHOULDER)
TORSO_PAIRS = ((R_SHOULDER, L_HIP), (L_SHOULDER, R_HIP), (R_SHOULDER, L_SHOULDER), (R_HIP, L_HIP))     # two diagonals, two widths
KEYPOINT_TABLES = {
    'cocoplus': list(range(NUM_KEYPOINTS)),
    'coco18': [10, 9, 8, 11, 12, 13, 4, 3, 2, 5, 6, 7, 1, -1, 0, 15, 14, 17, 16],
    'body25': [11, 10, 9, 12, 13, 14, 4, 3, 2, 5, 6, 7, 1, -1, 0, 16, 15, 18, 17],
}
KEYPOINT_COUNTS = {'cocoplus': 19, 'coco18': 18, 'body25': 25}
# (iterations, lr, l_theta, l_beta, l_s): entry 0 drives stage 1 (only its iterations, lr and l_s apply: neither the body pose nor the
# shape moves there), the others are the rounds of stage 2.  A documented default, not a tuned one.
DEFAULT_STAGES = ((100, 0.05, 0., 0., 1000.), (150, 0.02, 100., 100., 1000.), (150, 0.01, 10., 10., 1000.), (200, 0.005, 1., 1., 100.))
LAMBDA_3D = 1e4          # weight of the optional 3-D joint term: 0.01 units of error weigh like one pixel
# The silhouette term.  sigma: a vertex 20 px off the mask already weighs like an outlier (the keypoints' 100 px would let
# one stray limb outvote the contour); margin: half the spacing of the projected vertices -- SMPL's 6890 vertices on a body some 500 px
# tall and 150 px wide lie about 3.3 px apart, a body further away or a coarser model needs its own value; samples: contour samples per
# frame.  Documented defaults, not tuned ones.
DEFAULT_SILHOUETTE = {'sigma': 20., 'margin': 2., 'samples': 1024}
# (iterations, lr, l_theta, l_beta, l_s, l_in, l_cov): the rounds with the silhouette term, after stage 2.  Priors and step as in stage 2's
# last round; e_in and e_cov are means over vertices and samples, so l_in = 10 lets the mean inside residual weigh like ten keypoints and
# l_cov = 25 the mean coverage residual like twenty-five (the weights at which the float64 restatement recovers limbs without keypoints).
DEFAULT_SILHOUETTE_STAGES = ((100, 0.005, 1., 1., 100., 10., 25.),)
SAMPLE_FRAMES = 8        # frames per prefix sum while the contour samples are compacted
SilhouetteField = namedtuple('SilhouetteField', 'd2 samples counts')          # [F,H,W] int32, [F,S,2] int32 (x, y), [F] int32; on the GPU


# ---------------------------------------------------------------------------------------------- keypoints in, host side
def convert_keypoints(kp, fmt):
    """kp [F,K,3] = (x, y, confidence) in a detector's layout `fmt` ('cocoplus', 'coco18', 'body25') -> [F,19,3] float32 in the model's
    order; a joint the layout does not have (head top) gets confidence 0."""
    if fmt not in KEYPOINT_TABLES:
        raise ValueError(f"convert_keypoints: format {fmt!r}; known: {sorted(KEYPOINT_TABLES)}")
    kp = np.asarray(kp, np.float32)
    if kp.ndim != 3 or kp.shape[1:] != (KEYPOINT_COUNTS[fmt], 3):
        raise ValueError(f"convert_keypoints: {fmt} keypoints are [F,{KEYPOINT_COUNTS[fmt]},3], got {kp.shape}")
    out = np.zeros((kp.shape[0], NUM_KEYPOINTS, 3), np.float32)
    for k, src in enumerate(KEYPOINT_TABLES[fmt]):
        if src >= 0:
            out[:, k] = kp[:, src]
    return out


def read_keypoints(path, frames, fmt='cocoplus'):
    """[frames,19,3] float32 in the model's order from an `.npz` with `keypoints` [F,K,3] (F >= frames), or from a folder of OpenPose
    `*_keypoints.json` files, one per frame, ordered by the last integer in the stem: of each file the person with the highest summed
    confidence; a frame without a person has all confidences 0."""
    path = os.fspath(path)
    if os.path.isdir(path):
        files = glob.glob(os.path.join(path, '*_keypoints.json'))
        keyed = []
        for f in files:
            digits = re.findall(r'\d+', os.path.basename(f)[:-len('_keypoints.json')])
            if not digits:
                raise ValueError(f"{f}: no frame number in the file name")
            keyed.append((int(digits[-1]), f))
        keyed.sort()
        if len(keyed) < frames:
            raise ValueError(f"{path}: {len(keyed)} *_keypoints.json files for {frames} frames")
        if fmt not in KEYPOINT_COUNTS:
            raise ValueError(f"read_keypoints: format {fmt!r}; known: {sorted(KEYPOINT_TABLES)}")
        K = KEYPOINT_COUNTS[fmt]
        kp = np.zeros((frames, K, 3), np.float32)
        for i, (_, f) in enumerate(keyed[:frames]):
            with open(f, 'r') as fh:
                people = json.load(fh).get('people', [])
            best = None
            for person in people:
                flat = np.asarray(person.get('pose_keypoints_2d', []), np.float32)
                if flat.size != 3 * K:
                    raise ValueError(f"{f}: pose_keypoints_2d has {flat.size} numbers, {fmt} has {3 * K}")
                cand = flat.reshape(K, 3)
                if best is None or cand[:, 2].sum() > best[:, 2].sum():
                    best = cand
            if best is not None:
                kp[i] = best
    else:
        with np.load(path, allow_pickle=False) as data:
            if 'keypoints' not in data.files:
                raise ValueError(f"{path}: no `keypoints` array (has {data.files})")
            kp = np.asarray(data['keypoints'], np.float32)
        if kp.ndim != 3 or kp.shape[0] < frames:
            raise ValueError(f"{path}: keypoints {kp.shape} for {frames} frames")
        kp = kp[:frames]
    return convert_keypoints(kp, fmt)


# ---------------------------------------------------------------------------------------------- the camera and rotations, host side
def quat_to_matrix(q):
    """R [3,3] float64 of the quaternion (w, x, y, z) as CameraTableMixin.get_camera_parameters builds it."""
    q = np.asarray(q, np.float64).reshape(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z],
                     [2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x],
                     [2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z]])


def make_camera(R, T, fx, fy, cx, cy):
    """The camera as fit_sequence takes it: pc = p R + T, x = cx - fx pc_x / pc_z, y = cy - fy pc_y / pc_z (CameraMine.project)."""
    return {'R': np.asarray(R, np.float64).reshape(3, 3), 'T': np.asarray(T, np.float64).reshape(3), 'fx': float(fx), 'fy': float(fy),
            'cx': float(cx), 'cy': float(cy)}


def read_camera(path):
    """make_camera from a capture folder's `camera.npz` (fx, fy, cx, cy, quat, T), as read_scene_folder reads it."""
    with np.load(path) as data:
        return make_camera(quat_to_matrix(data['quat']), data['T'], data['fx'], data['fy'], data['cx'], data['cy'])


def camera_floats(camera):
    return [float(v) for v in camera['R'].reshape(-1)] + [float(v) for v in camera['T']] + [camera['fx'], camera['fy'], camera['cx'], camera['cy']]


def matrix_to_axis_angle(R):
    """Axis-angle [3] of a rotation matrix through its quaternion (stable up to a half turn)."""
    R = np.asarray(R, np.float64)
    q = np.array([1.0 + R[0, 0] + R[1, 1] + R[2, 2], 1.0 + R[0, 0] - R[1, 1] - R[2, 2], 1.0 - R[0, 0] + R[1, 1] - R[2, 2], 1.0 - R[0, 0] - R[1, 1] + R[2, 2]])
    i = int(np.argmax(q))
    if i == 0:
        q = np.array([q[0], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif i == 1:
        q = np.array([R[2, 1] - R[1, 2], q[1], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif i == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], q[2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], q[3]])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    s = np.linalg.norm(q[1:])
    if s < 1e-12:
        return np.zeros(3)
    return q[1:] / s * (2.0 * np.arctan2(s, q[0]))


def default_starts(camera):
    """[2,3] axis-angle root orientations in the world: the body as the camera sees it from behind (the identity in the camera's frame,
    +x left, +y up, +z forward) and facing the camera (the half turn about the camera's vertical axis), both taken through the camera's R."""
    half_turn = np.diag([-1.0, 1.0, -1.0])
    return np.stack([matrix_to_axis_angle(camera['R']), matrix_to_axis_angle(camera['R'] @ half_turn)])


# ---------------------------------------------------------------------------------------------- stage 0
def initial_translation(keypoints, joints0, camera):
    """trans [F,3] float64 in closed form.  Per frame the depth is the median, over the torso pairs with both ends confident, of
    (3-D length of the pair in the zero pose joints0 [K,3]) / (its 2-D length in focal units) -- the pinhole relation for a segment
    parallel to the image plane -- and x, y put the hip centre on the ray through its 2-D position.  A frame with fewer than two
    confident pairs takes the value of the nearest frame that has them (the earlier one on a tie)."""
    kp = np.asarray(keypoints, np.float64)
    J0 = np.asarray(joints0, np.float64)
    F = kp.shape[0]
    ok_joint = np.isfinite(kp).all(-1) & (kp[..., 2] > 0)
    trans = np.zeros((F, 3))
    good = np.zeros(F, bool)
    hip0 = 0.5 * (J0[R_HIP] + J0[L_HIP])
    Rinv = camera['R'].T
    for t in range(F):
        depths = []
        for a, b in TORSO_PAIRS:
            if ok_joint[t, a] and ok_joint[t, b]:
                d2 = np.hypot((kp[t, a, 0] - kp[t, b, 0]) / camera['fx'], (kp[t, a, 1] - kp[t, b, 1]) / camera['fy'])
                if d2 > 0:
                    depths.append(np.linalg.norm(J0[a] - J0[b]) / d2)
        if len(depths) < 2 or not (ok_joint[t, R_HIP] and ok_joint[t, L_HIP]):
            continue
        z = float(np.median(depths))
        u, v = 0.5 * (kp[t, R_HIP, :2] + kp[t, L_HIP, :2])
        pc = np.array([(camera['cx'] - u) * z / camera['fx'], (camera['cy'] - v) * z / camera['fy'], z])
        trans[t] = (pc - camera['T']) @ Rinv - hip0
        good[t] = True
    if not good.any():
        raise ValueError("initial_translation: no frame has two confident torso pairs and both hips")
    idx = np.flatnonzero(good)
    for t in np.flatnonzero(~good):
        trans[t] = trans[idx[np.argmin(np.abs(idx - t))]]
    return trans


# ---------------------------------------------------------------------------------------------- the energy
class _KeypointEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, joints, trans, kp, joint_weights, camera, sigma):
        energy, g_joints, g_trans, behind = ops.keypoint_energy(joints.contiguous(), trans.contiguous(), kp, joint_weights, camera, sigma)
        ctx.save_for_backward(g_joints, g_trans)
        ctx.mark_non_differentiable(behind)
        return energy, behind

    @staticmethod
    def backward(ctx, g_energy, _):
        g_joints, g_trans = ctx.saved_tensors
        return g_joints * g_energy.view(-1, 1, 1), g_trans * g_energy.view(-1, 1), None, None, None, None


def keypoint_energy(joints, trans, kp, joint_weights, camera, sigma):
    """(energy [T], behind [T] int32), differentiable in joints [T,K,3] and trans [T,3]; camera: camera_floats(...)."""
    return _KeypointEnergy.apply(joints, trans, kp, joint_weights, camera, sigma)


# ---------------------------------------------------------------------------------------------- the silhouette term
def _masks_on(masks, device):
    m = masks if torch.is_tensor(masks) else torch.from_numpy(np.ascontiguousarray(np.asarray(masks)))
    if m.dim() != 3 or m.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"masks are [F,H,W] uint8 or bool, got {m.dtype} {tuple(m.shape)}")
    if device is None:
        device = m.device if m.is_cuda else torch.device('cuda', torch.cuda.current_device())
    return m.to(device)


def distance_transform(masks, device=None):
    """d2 [F,H,W] int32 on the GPU: of every pixel the exact squared distance, in pixels, to the nearest non-zero pixel of the same frame
    of masks [F,H,W] (uint8 or bool, host or device); 0 on the mask.  A frame without any mask pixel holds ops.EDT_EMPTY = 1 << 30 in
    every entry.  H, W <= 8192, so that the squared diagonal stays inside int32."""
    return ops.edt(_masks_on(masks, device))


def contour_samples(masks, samples):
    """(samples [F,S,2] int32 = (x, y), counts [F] int32) on the masks' device (the GPU).  A contour pixel is a mask pixel with a
    4-neighbour inside the image that is background (the image's border makes none: a body cropped by the frame has no edge there).
    Of a frame's n contour pixels in row-major order all are taken when n <= S, else pixel floor(i n / S) for i < S (int64); counts
    holds n, the rows past min(n, S) are zero.  Flags from sr_contour_flags, then a prefix sum and a binary search per frame: no host read."""
    S = int(samples)
    if S < 1 or S > ops.SIL_MAX_SAMPLES:
        raise ValueError(f"contour_samples: 1 <= samples <= {ops.SIL_MAX_SAMPLES}, got {samples}")
    flags = ops.contour_flags(masks)
    F, H, W = flags.shape
    dev = flags.device
    out = torch.zeros((F, S, 2), dtype=torch.int32, device=dev)
    counts = torch.empty((F,), dtype=torch.int32, device=dev)
    i = torch.arange(S, dtype=torch.int64, device=dev).view(1, S)
    for f0 in range(0, F, SAMPLE_FRAMES):
        cum = torch.cumsum(flags[f0:f0 + SAMPLE_FRAMES].view(-1, H * W), 1, dtype=torch.int32)          # inclusive ranks, H W < 2^31
        n = cum[:, -1].to(torch.int64).view(-1, 1)
        rank = torch.where(n <= S, i, (i * n) // S)
        live = i < n.clamp(max=S)
        pos = torch.searchsorted(cum, (rank + 1).to(torch.int32))                                       # the first pixel whose rank is rank + 1
        pos = torch.where(live, pos, torch.zeros_like(pos))
        out[f0:f0 + SAMPLE_FRAMES, :, 0] = (pos % W).to(torch.int32)
        out[f0:f0 + SAMPLE_FRAMES, :, 1] = (pos // W).to(torch.int32)
        counts[f0:f0 + SAMPLE_FRAMES] = cum[:, -1]
    return out, counts


def silhouette_field(masks, samples=DEFAULT_SILHOUETTE['samples'], device=None):
    """SilhouetteField(d2, samples, counts) of masks [F,H,W] (uint8 or bool, host or device), on the GPU: what silhouette_energy reads."""
    m = _masks_on(masks, device)
    return SilhouetteField(ops.edt(m), *contour_samples(m, samples))


class _SilhouetteEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, d2, samples, counts, camera, sigma, margin):
        e_in, e_cov, outside, g_points, _ = ops.silhouette_energy(points.contiguous(), d2, samples, counts, camera, sigma, margin)
        ctx.save_for_backward(g_points)
        ctx.mark_non_differentiable(outside)
        return e_in, e_cov, outside

    @staticmethod
    def backward(ctx, g_in, g_cov, _):
        g_points, = ctx.saved_tensors
        return torch.addcmul(g_points[0] * g_in.view(-1, 1, 1), g_points[1], g_cov.view(-1, 1, 1)), None, None, None, None, None, None


def silhouette_energy(points, field, camera, sigma=DEFAULT_SILHOUETTE['sigma'], margin=DEFAULT_SILHOUETTE['margin']):
    """(e_in [F], e_cov [F], outside [F] int32), differentiable in points [F,V,3] (world positions, the translation added); field:
    silhouette_field(...); camera: camera_floats(...).  e_in[t] = mean_v rho_sigma(d(project(p_tv))) with d the bilinear interpolation of
    the distance field, e_cov[t] = mean_s rho_sigma(max(0, min_v |c_ts - project(p_tv)| - margin)) with the match held fixed in the
    gradient; outside counts the vertices behind the camera, off the image or non-finite, which add nothing to e_in."""
    return _SilhouetteEnergy.apply(points, field.d2, field.samples, field.counts, camera, sigma, margin)


def silhouette_residuals(points, field, camera, margin):
    """(inside [F], cover [F]) float32: the two terms' mean residuals in pixels, without the robustifier -- the mean of d over the
    vertices inside the image and the mean of max(0, distance to the matched vertex - margin) over the samples in use (0 for a frame
    without either).  The matches are the kernel's; the means are torch operators: this is the report, not the loop."""
    with torch.no_grad():
        pts = points.detach().contiguous()
        _, _, _, _, match = ops.silhouette_energy(pts, field.d2, field.samples, field.counts, camera, 1., margin)
        R = torch.tensor(camera[:9], dtype=torch.float32, device=pts.device).view(3, 3)
        T = torch.tensor(camera[9:12], dtype=torch.float32, device=pts.device)
        pc = pts.matmul(R) + T
        front = pc[..., 2] > 0
        z = torch.where(front, pc[..., 2], torch.ones_like(pc[..., 2]))
        xy = torch.stack([camera[14] - camera[12] * pc[..., 0] / z, camera[15] - camera[13] * pc[..., 1] / z], -1)
        F, H, W = field.d2.shape
        ok = front & torch.isfinite(xy).all(-1) & (xy[..., 0] >= 0) & (xy[..., 0] <= W - 1) & (xy[..., 1] >= 0) & (xy[..., 1] <= H - 1)
        ok &= (field.d2[:, 0, 0] != ops.EDT_EMPTY).view(F, 1)
        x = torch.where(ok, xy[..., 0], torch.zeros_like(z))
        y = torch.where(ok, xy[..., 1], torch.zeros_like(z))
        x0, y0 = x.floor().clamp(0, W - 2).long(), y.floor().clamp(0, H - 2).long()
        fx, fy = x - x0, y - y0
        flat = field.d2.view(F, H * W)
        tap = lambda dy, dx: torch.gather(flat, 1, (y0 + dy) * W + x0 + dx).float().sqrt()          # noqa: E731
        d = (tap(0, 0) * (1 - fx) + tap(0, 1) * fx) * (1 - fy) + (tap(1, 0) * (1 - fx) + tap(1, 1) * fx) * fy
        inside = torch.where(ok, d, torch.zeros_like(d)).sum(1) / ok.sum(1).clamp(min=1)
        S = field.samples.shape[1]
        used = (torch.arange(S, device=pts.device).view(1, S) < field.counts.clamp(max=S).view(F, 1)) & (match >= 0)
        hit = torch.gather(xy, 1, match.clamp(min=0).long().unsqueeze(-1).expand(F, S, 2))
        r = ((hit - field.samples.float()).norm(dim=-1) - margin).clamp(min=0)
        cover = torch.where(used, r, torch.zeros_like(r)).sum(1) / field.counts.clamp(min=1, max=S)
    return inside, cover


def mask_error(smpl, points, masks, camera):
    """[F]: 1 - IoU of the rasterised body (points [F,V,3] with the model's faces) against masks [F,H,W] on the GPU, through
    posed.rasterize_posed and posed.mask_iou_error; None when the image is not square (the rasteriser's limit) or the model has no faces."""
    from . import posed
    from .model.CameraMine import RectifiedPerspectiveCameras
    F, H, W = masks.shape
    faces = getattr(smpl, 'faces_tensor', None)
    if H != W or faces is None or faces.numel() == 0:
        return None
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=points.device)          # noqa: E731
    cams = RectifiedPerspectiveCameras(f32([camera['fx'], camera['fy']]), f32([camera['cx'], camera['cy']]), f32(camera['R']), f32(camera['T']), [(W, H)])
    frags, _ = posed.rasterize_posed(points.detach().contiguous(), faces.to(points.device), cams, H, W)
    return posed.mask_iou_error((frags.pix_to_face[..., 0] >= 0).float(), (masks != 0).float())


def _energy(smpl, root, body, trans, beta, kp, jw, cam, sigma, l_theta, l_beta, l_s, joints3d, l_3, sil=None):
    F = root.shape[0]
    theta = torch.cat([root.view(F, 1, 3), body], 1)
    if sil is None:
        joints = smpl(beta.expand(F, -1), theta)
    else:                                                 # (field, sigma, margin, l_in, l_cov): the vertices of the same forward
        verts, joints, _ = smpl(beta.expand(F, -1), theta, get_skin=True)
    e_kp, _ = keypoint_energy(joints, trans, kp, jw, cam, sigma)
    E = e_kp.sum()
    if sil is not None:
        e_in, e_cov, _ = silhouette_energy(verts + trans.view(F, 1, 3), sil[0], cam, sil[1], sil[2])
        E = E + sil[3] * e_in.sum() + sil[4] * e_cov.sum()
    if l_theta:
        E = E + l_theta * (body ** 2).sum()
    if l_beta:
        E = E + l_beta * (beta ** 2).sum()
    if (l_s and F > 1) or joints3d is not None:
        J3 = joints + trans.view(F, 1, 3)
        if l_s and F > 1:
            E = E + l_s * ((J3[1:] - J3[:-1]) ** 2).sum()
        if joints3d is not None:
            E = E + l_3 * ((J3 - joints3d) ** 2).sum()
    return E, e_kp


def _descend(smpl, params, frozen, iters, lr, history, offset, energy_args):
    """`iters` FusedAdam steps on the tensors named in `params` (the others stay as they are); energies go to history[offset:...]."""
    state = dict(frozen)
    for name, value in params.items():
        state[name] = value.detach().clone().requires_grad_(True)
    opt = FusedAdam([state[name] for name in params], lr=lr)
    for it in range(iters):
        opt.zero_grad(set_to_none=True)
        E, _ = _energy(smpl, state['root'], state['body'], state['trans'], state['beta'], *energy_args)
        history[offset + it].copy_(E.detach())
        E.backward()
        opt.step()
    return {name: state[name].detach() for name in state}


def fit_sequence(smpl, keypoints, camera, *, joints3d=None, init=None, gender='neutral', sigma=100., stages=DEFAULT_STAGES, joint_weights=None,
                 starts=None, seed=0, lambda_3d=LAMBDA_3D, masks=None, silhouette=None, silhouette_stages=DEFAULT_SILHOUETTE_STAGES):
    """Fit `smpl` (a DifferentiableSMPL with the 19 cocoplus joints, on the GPU) to keypoints [F,19,3] = (x, y, confidence) under
    `camera` (make_camera / read_camera).  -> dict: poses [F,24,3], shape [10], trans [F,3] float32 numpy; reproj [F] (mean pixel
    error over the joints with confidence > 0), behind [F] (joints behind the camera), history (the energy of every iteration, in
    order: stage 1 per start, then the rounds of stage 2; read once, at the end), start (the index of the winning start), gender.

    joints3d [F,19,3] adds lambda_3d sum |J3d - joints3d|^2 (joint positions in the world, translation included) -- for converting or
    refining the output of another estimator.  init (a dict or npz path with poses, shape, trans) replaces stages 0 and 1.
    joint_weights [19] scale the 2-D term per joint (default ones).  starts [S,3]: the root orientations stage 1 tries (default_starts).
    `seed` is accepted for interface stability only: the fit draws no random numbers.

    masks [F,H,W] (uint8 or bool, host or device) adds the silhouette term: after stage 2 the rounds of silhouette_stages =
    (iterations, lr, l_theta, l_beta, l_s, l_in, l_cov) minimise the energy above plus l_in sum_t e_in[t] + l_cov sum_t e_cov[t]
    (silhouette_energy) over all parameters; `silhouette` overrides entries of DEFAULT_SILHOUETTE (sigma, margin, samples).  history
    grows by those iterations and the result gains sil_inside [F], sil_cover [F] (the two terms' mean residuals in pixels at the end,
    silhouette_residuals), sil_outside [F] (vertices that are behind the camera, off the image or non-finite), sil_empty (the number of
    frames without a mask pixel: they take no part in the term) and mask_error ([F] 1 - IoU of the rasterised body, or None: mask_error).
    Without masks nothing changes: the same operators run and the result has the same keys."""
    dev = smpl.v_template.device
    if smpl.joint_regressor.shape[1] != NUM_KEYPOINTS:
        raise ValueError("fit_sequence: the body model must regress the 19 cocoplus joints (joint_type='cocoplus')")
    kp_host = np.asarray(keypoints, np.float32)
    if kp_host.ndim != 3 or kp_host.shape[1:] != (NUM_KEYPOINTS, 3):
        raise ValueError(f"fit_sequence: keypoints are [F,19,3], got {kp_host.shape}")
    F = kp_host.shape[0]
    stages = tuple(tuple(s) for s in stages)
    if len(stages) < 1 or any(len(s) != 5 for s in stages):
        raise ValueError("fit_sequence: stages is a tuple of (iterations, lr, l_theta, l_beta, l_s), entry 0 for stage 1")
    kp = torch.from_numpy(np.ascontiguousarray(kp_host)).to(dev)
    jw_host = np.ones(NUM_KEYPOINTS, np.float32) if joint_weights is None else np.asarray(joint_weights, np.float32).reshape(NUM_KEYPOINTS)
    jw = torch.from_numpy(jw_host).to(dev)
    torso_host = np.zeros(NUM_KEYPOINTS, np.float32)
    torso_host[list(TORSO)] = jw_host[list(TORSO)]
    jw_torso = torch.from_numpy(torso_host).to(dev)
    cam = camera_floats(camera)
    target3d = None if joints3d is None else torch.from_numpy(np.ascontiguousarray(np.asarray(joints3d, np.float32))).to(dev)
    if target3d is not None and tuple(target3d.shape) != (F, NUM_KEYPOINTS, 3):
        raise ValueError(f"fit_sequence: joints3d is [F,19,3], got {tuple(target3d.shape)}")
    nbeta = smpl.num_betas
    zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)          # noqa: E731
    starts_host = default_starts(camera) if starts is None else np.asarray(starts, np.float64).reshape(-1, 3)
    field = None
    if masks is not None:
        unknown = set(silhouette or {}) - set(DEFAULT_SILHOUETTE)
        if unknown:
            raise ValueError(f"fit_sequence: silhouette has {sorted(unknown)}; known: {sorted(DEFAULT_SILHOUETTE)}")
        sil_cfg = dict(DEFAULT_SILHOUETTE, **(silhouette or {}))
        sil_stages = tuple(tuple(s) for s in silhouette_stages)
        if any(len(s) != 7 for s in sil_stages):
            raise ValueError("fit_sequence: silhouette_stages is a tuple of (iterations, lr, l_theta, l_beta, l_s, l_in, l_cov)")
        masks_dev = _masks_on(masks, dev)
        if masks_dev.shape[0] != F:
            raise ValueError(f"fit_sequence: masks {tuple(masks_dev.shape)} for {F} frames")
        field = silhouette_field(masks_dev, sil_cfg['samples'])
    else:
        sil_stages = ()
    history = zeros(sum(s[0] for s in stages[1:]) + (0 if init is not None else stages[0][0] * starts_host.shape[0]) + sum(s[0] for s in sil_stages))
    start_index = torch.zeros((), dtype=torch.int64, device=dev)
    done = 0
    if init is not None:
        if not isinstance(init, dict):
            with np.load(os.fspath(init)) as data:
                init = {k: data[k] for k in ('poses', 'shape', 'trans')}
        poses0 = torch.from_numpy(np.asarray(init['poses'], np.float32).reshape(-1, 24, 3)[:F].copy()).to(dev)
        state = {'root': poses0[:, 0].contiguous(), 'body': poses0[:, 1:].contiguous(),
                 'trans': torch.from_numpy(np.asarray(init['trans'], np.float32).reshape(-1, 3)[:F].copy()).to(dev),
                 'beta': torch.from_numpy(np.asarray(init['shape'], np.float32).reshape(1, -1)[:, :nbeta].copy()).to(dev)}
        if state['root'].shape[0] != F or state['trans'].shape[0] != F:
            raise ValueError(f"fit_sequence: init holds fewer than {F} frames")
    else:
        with torch.no_grad():
            joints0 = smpl(zeros(1, nbeta), zeros(1, 24, 3))[0].double().cpu().numpy()
        trans0 = torch.from_numpy(initial_translation(kp_host, joints0, camera).astype(np.float32)).to(dev)
        iters, lr, _, _, l_s = stages[0]
        results, totals = [], []
        for s in range(starts_host.shape[0]):
            root0 = torch.from_numpy(starts_host[s].astype(np.float32)).to(dev).view(1, 3).repeat(F, 1)
            frozen = {'body': zeros(F, 23, 3), 'beta': zeros(1, nbeta)}
            args = (kp, jw_torso, cam, sigma, 0., 0., l_s, None, 0.)
            out = _descend(smpl, {'root': root0, 'trans': trans0}, frozen, iters, lr, history, done, args)
            done += iters
            with torch.no_grad():
                totals.append(_energy(smpl, out['root'], out['body'], out['trans'], out['beta'], *args)[0])
            results.append(out)
        start_index = torch.argmin(torch.stack(totals))                              # (stays on the device; the first of equal energies)
        state = {name: torch.index_select(torch.stack([r[name] for r in results]), 0, start_index.view(1))[0] for name in results[0]}
    for iters, lr, l_theta, l_beta, l_s in stages[1:]:
        args = (kp, jw, cam, sigma, l_theta, l_beta, l_s, target3d, lambda_3d)
        state = _descend(smpl, dict(state), {}, iters, lr, history, done, args)
        done += iters
    for iters, lr, l_theta, l_beta, l_s, l_in, l_cov in sil_stages:
        args = (kp, jw, cam, sigma, l_theta, l_beta, l_s, target3d, lambda_3d, (field, sil_cfg['sigma'], sil_cfg['margin'], l_in, l_cov))
        state = _descend(smpl, dict(state), {}, iters, lr, history, done, args)
        done += iters
    with torch.no_grad():
        theta = torch.cat([state['root'].view(F, 1, 3), state['body']], 1)
        if field is None:
            joints = smpl(state['beta'].expand(F, -1).contiguous(), theta)
        else:
            verts, joints, _ = smpl(state['beta'].expand(F, -1).contiguous(), theta, get_skin=True)
        _, behind = keypoint_energy(joints, state['trans'], kp, jw, cam, sigma)
        reproj = reprojection_error(joints + state['trans'].view(F, 1, 3), kp, camera)
    result = {'poses': theta.cpu().numpy(), 'shape': state['beta'].view(-1).cpu().numpy(), 'trans': state['trans'].cpu().numpy(),
              'reproj': reproj.cpu().numpy(), 'behind': behind.cpu().numpy(), 'history': history.cpu().numpy(), 'start': int(start_index),
              'gender': str(gender)}
    if field is not None:
        with torch.no_grad():
            points = (verts + state['trans'].view(F, 1, 3)).contiguous()
            _, _, outside = silhouette_energy(points, field, cam, sil_cfg['sigma'], sil_cfg['margin'])
            inside, cover = silhouette_residuals(points, field, cam, sil_cfg['margin'])
            err = mask_error(smpl, points, masks_dev, camera)
        result.update({'sil_inside': inside.cpu().numpy(), 'sil_cover': cover.cpu().numpy(), 'sil_outside': outside.cpu().numpy(),
                       'sil_empty': int((field.d2[:, 0, 0] == ops.EDT_EMPTY).sum()), 'mask_error': None if err is None else err.cpu().numpy()})
    return result


def reprojection_error(points, kp, camera):
    """[F] mean pixel distance between the projections of points [F,K,3] (world, float32) and kp [F,K,3] over the joints with a finite
    target and confidence > 0 (0 for a frame without any); torch, on the tensors' device."""
    from .model.CameraMine import RectifiedPerspectiveCameras
    f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32), device=points.device)          # noqa: E731
    cams = RectifiedPerspectiveCameras(f32([camera['fx'], camera['fy']]), f32([camera['cx'], camera['cy']]), f32(camera['R']), f32(camera['T']), (0, 0))
    xy, _ = cams.project(points)
    ok = torch.isfinite(kp).all(-1) & (kp[..., 2] > 0)
    tgt = torch.where(ok.unsqueeze(-1), kp, torch.zeros_like(kp))
    d = torch.where(ok, (xy - tgt[..., :2]).norm(dim=-1), torch.zeros_like(xy[..., 0]))
    return d.sum(-1) / ok.sum(-1).clamp(min=1)
