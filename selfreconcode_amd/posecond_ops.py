"""Operators of the pose conditioning (csrc/posecond.hip): GPU tensors only, no autograd.  `animate.py` is the public
interface.  A pose's feature is SMPL's pose feature without the root joint (R_j - I, joints 1 .. 23); the neighbours of a pose are the
training frames with the smallest squared feature distance; a code for the pose is their codes' Gaussian-weighted mean.  Two calls
give identical bits.

The entry points are declared in csrc/posecond_abi.h and bound here (_lib.bind_header): a library without them fails this import."""
import math
import os

import torch

from . import _lib
from .build import CSRC

_DEFINES, _ = _lib.bind_header(os.path.join(CSRC, "posecond_abi.h"))
JOINTS = _DEFINES["SR_POSE_JOINTS"]                       # the joints of the feature: 1 .. 23
FEATS = _DEFINES["SR_POSE_FEATS"]
MAX_K = _DEFINES["SR_POSE_MAX_K"]
LD_ALIGN = 64                                             # columns of a feature matrix: the count rounded up to this


def _theta(poses, who):
    """poses [N,24,3] or [N,72] -> float32 contiguous [N,24,3] on the GPU."""
    _lib.require_gpu(poses)
    if poses.dim() == 2 and poses.shape[1] == 72:
        poses = poses.reshape(-1, 24, 3)
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (24, 3) or poses.shape[0] == 0:
        raise ValueError(f"{who}: poses [N,24,3] or [N,72] with N > 0 expected, got {tuple(poses.shape)}")
    return _lib.f32c(poses)


def _scale(joint_weights, device):
    """sqrt(w) [23] float32 on `device` (None: None) of joint weights w_j >= 0 for joints 1 .. 23."""
    if joint_weights is None:
        return None
    w = torch.as_tensor(joint_weights, dtype=torch.float32).reshape(-1)
    if w.numel() != JOINTS or not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
        raise ValueError(f"joint_weights: {JOINTS} finite values >= 0 expected (joints 1 .. {JOINTS})")
    return w.sqrt().to(device).contiguous()


def _features(theta, scale):
    N = theta.shape[0]
    ld = -(-N // LD_ALIGN) * LD_ALIGN
    feat_t = torch.zeros((FEATS, ld), dtype=torch.float32, device=theta.device)
    _lib.launch("sr_pose_features", theta, theta, N, scale, feat_t, ld)
    return feat_t


def pose_features(theta, joint_weights=None):
    """feat_t [207, ld] float32, ld = N rounded up to LD_ALIGN: column n < N is the feature of pose theta[n] ([N,24,3] or [N,72],
    axis-angle) -- the entries of R_j - I for joints 1 .. 23, each joint's nine multiplied by sqrt(joint_weights[j - 1]) -- and the
    columns past N are zero.  The root joint is left out: global orientation says nothing about cloth."""
    theta = _theta(theta, "pose_features")
    return _features(theta, _scale(joint_weights, theta.device))


class PoseIndex:
    """The training poses as the search reads them: `feat_t` [207, ld] (pose_features), `N`, and `scale` (sqrt of the joint weights, or
    None), which the queries' features are made with."""

    def __init__(self, feat_t, N, scale):
        self.feat_t, self.N, self.scale = feat_t, int(N), scale

    @classmethod
    def build(cls, train_poses, joint_weights=None):
        theta = _theta(train_poses, "PoseIndex.build")
        scale = _scale(joint_weights, theta.device)
        return cls(_features(theta, scale), theta.shape[0], scale)


def _frames(query_frames, Q, device):
    if query_frames is None:
        return None
    frames = torch.as_tensor(query_frames, device=device).reshape(-1).to(torch.int32).contiguous()
    if frames.numel() != Q:
        raise ValueError(f"pose_neighbors: {Q} query_frames expected, got {frames.numel()}")
    return frames


def feature_neighbors(featq_t, Q, index, K=4, query_frames=None, exclude=-1, method="fused"):
    """pose_neighbors for queries given as features (featq_t [207, ldq], the first Q columns)."""
    K, exclude = int(K), int(exclude)
    if not 1 <= K <= MAX_K:
        raise ValueError(f"pose_neighbors: K in [1, {MAX_K}] expected, got {K}")
    if method not in ("fused", "matrix"):
        raise ValueError(f"method must be 'fused' or 'matrix', got {method!r}")
    dev, N = featq_t.device, index.N
    frames = _frames(query_frames, Q, dev)
    if method == "fused":
        idx = torch.empty((Q, K), dtype=torch.int32, device=dev)
        d2 = torch.empty((Q, K), dtype=torch.float32, device=dev)
        _lib.launch("sr_pose_neighbors", featq_t, featq_t, featq_t.shape[1], Q, index.feat_t, index.feat_t.shape[1], N, K, frames, exclude, idx, d2)
        return idx, d2
    D = torch.empty((Q, N), dtype=torch.float32, device=dev)
    _lib.launch("sr_pose_dist", featq_t, featq_t, featq_t.shape[1], Q, index.feat_t, index.feat_t.shape[1], N, D)
    inf = D.new_tensor(math.inf)
    D = torch.where(torch.isfinite(D), D, inf)
    if frames is not None and exclude >= 0:
        near = (torch.arange(N, device=dev)[None, :] - frames.long()[:, None]).abs() <= exclude
        D = torch.where(near, inf, D)
    d2, idx = torch.sort(D, dim=1, stable=True)                               # ties: the lower frame first
    d2, idx = d2[:, :K], idx[:, :K].to(torch.int32)
    idx = torch.where(torch.isinf(d2), torch.full_like(idx, -1), idx)
    if N < K:
        d2 = torch.cat([d2, d2.new_full((Q, K - N), math.inf)], dim=1)
        idx = torch.cat([idx, idx.new_full((Q, K - N), -1)], dim=1)
    return idx.contiguous(), d2.contiguous()


def pose_neighbors(query_poses, index, K=4, query_frames=None, exclude=-1, method="fused"):
    """(idx [Q,K] int32, d2 [Q,K] float32): for each query pose the K training frames of `index` with the smallest
    d2 = sum_e (phi_q[e] - phi_n[e])^2 (float32, e ascending, fused multiply-add), in ascending (d2, frame) order.  With `query_frames`
    [Q] and exclude >= 0, frame n is no candidate of query q when |n - query_frames[q]| <= exclude; a frame with a non-finite d2 is
    none ever.  Slots without a candidate hold idx -1, d2 +inf.  method "fused" is one launch (sr_pose_neighbors); "matrix" is the
    witness: the full matrix (sr_pose_dist), the exclusion as +inf and torch's stable sort -- the same bits."""
    theta = _theta(query_poses, "pose_neighbors")
    if theta.device != index.feat_t.device:
        raise ValueError(f"pose_neighbors: queries on {theta.device}, index on {index.feat_t.device}")
    return feature_neighbors(_features(theta, index.scale), theta.shape[0], index, K, query_frames, exclude, method)


def blend_codes(idx, d2, codes, sigma2):
    """(codes_q [Q,L], weights [Q,K]) from pose_neighbors' idx / d2 and the training codes [N,L]: w_k = exp(-(d2_k - d2_0) / (2 sigma2))
    over the filled slots, normalised by their sum (ascending k); codes_q = sum_k w_k codes[idx_k] (ascending k, fused multiply-add).
    A row without a filled slot gives zeros.  `sigma2` > 0 with a finite float32 1 / (2 sigma2)."""
    _lib.require_gpu(idx, d2, codes)
    if idx.dim() != 2 or tuple(d2.shape) != tuple(idx.shape) or not 1 <= idx.shape[1] <= MAX_K or idx.shape[0] == 0:
        raise ValueError(f"blend_codes: idx / d2 [Q,K] with K in [1, {MAX_K}] expected, got {tuple(idx.shape)} / {tuple(d2.shape)}")
    if codes.dim() != 2 or codes.shape[0] == 0 or codes.shape[1] == 0:
        raise ValueError(f"blend_codes: codes [N,L] expected, got {tuple(codes.shape)}")
    sigma2 = float(sigma2)
    inv = float(torch.tensor(0.5 / sigma2, dtype=torch.float32)) if sigma2 > 0. else math.nan
    if not math.isfinite(inv):
        raise ValueError(f"blend_codes: sigma2 > 0 with a finite float32 1 / (2 sigma2) expected, got {sigma2}")
    idx, d2, codes = idx.to(torch.int32).contiguous(), _lib.f32c(d2), _lib.f32c(codes)
    Q, K = idx.shape
    out = torch.empty((Q, codes.shape[1]), dtype=torch.float32, device=codes.device)
    weights = torch.empty((Q, K), dtype=torch.float32, device=codes.device)
    _lib.launch("sr_code_blend", codes, idx, d2, Q, K, inv, codes, codes.shape[0], codes.shape[1], out, weights)
    return out, weights


def lower_median(values):
    """The lower median of a 1-D tensor with at least one element (element (m - 1) // 2 of the sorted values), as a tensor."""
    return torch.sort(values)[0][(values.numel() - 1) // 2]


def calibrate_sigma2(index, exclude):
    """sigma^2 for blend_codes from the training poses alone: the lower median, over the training frames that have a candidate, of d2 to
    their nearest training frame outside +-exclude.  One search with query_frames = arange(N).  ValueError when no frame has a
    candidate (the window covers the capture) or the median is 0 (repeated poses): pass an explicit sigma then."""
    N = index.N
    _, d2 = feature_neighbors(index.feat_t, N, index, 1, torch.arange(N, device=index.feat_t.device), int(exclude), "fused")
    d2 = d2[:, 0]
    d2 = d2[torch.isfinite(d2)]
    if d2.numel() == 0:
        raise ValueError(f"calibrate_sigma2: no training frame has a neighbour outside +-{int(exclude)} frames among {N}; pass an explicit sigma")
    sigma2 = float(lower_median(d2))
    if not sigma2 > 0.:
        raise ValueError("calibrate_sigma2: the median nearest-pose distance is 0 (repeated poses); pass an explicit sigma")
    return sigma2
