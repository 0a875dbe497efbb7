"""float64 numpy twin of the skinning-field builder (compute_lbswField + smooth_weights, model/Deformer.py:235-284 of the reference): the
same formulas, restated, in double.  tools/gen_lbsw_golden.py measures the reference's own float32 result against it and records the
error; the tests measure ours against it and allow 4x that (floor 1e-6)."""
import numpy as np

GOLDEN_BODY_SEED = 0
K_REF = 30
SMALL_GRID = (17, 29, 9)          # (W, H, D), three distinct odd sizes: any transposition changes the shape
MID_GRID = (33, 57, 17)
MID_STRIDE = 37                   # voxels MID_STRIDE // 2 :: MID_STRIDE of the flattened (D, H, W) order
GAP_MIN = 1e-6                    # voxels whose k-th and (k+1)-th distances are closer than this (relative) may be left out ...
EXCLUDE_CAP = 1e-3                # ... at most this share of them


def centres(bmin, bmax, res, align_corners=False, flat_index=None):
    """Voxel centres [n,3] (x, y, z) of the (W, H, D) grid in flattened (D, H, W) order, or of the voxels `flat_index` of it."""
    W, H, D = res
    idx = np.arange(W * H * D) if flat_index is None else np.asarray(flat_index)
    ijk = np.stack([idx % W, (idx // W) % H, idx // (W * H)], -1).astype(np.float64)
    r = np.array([W, H, D], np.float64)
    u = ijk / (r - 1) if align_corners else (ijk + 0.5) / r
    lo, hi = np.asarray(bmin, np.float32).astype(np.float64), np.asarray(bmax, np.float32).astype(np.float64)
    return u * (hi - lo) + lo


def knn_blend(points, verts, vws, k, chunk=2048):
    """(blend [n,nj], gap [n]) in float64: inverse-distance blend over the k nearest vertices (distances clamped to [1e-4, 1]), and the
    relative gap (d_{k+1} - d_k) / d_{k+1} between the last neighbour taken and the first one left out (inf when k = nv)."""
    v, ws = np.asarray(verts, np.float32).astype(np.float64), np.asarray(vws, np.float32).astype(np.float64)
    nv = v.shape[0]
    out, gap = np.empty((points.shape[0], ws.shape[1])), np.full((points.shape[0],), np.inf)
    for s in range(0, points.shape[0], chunk):
        p = points[s:s + chunk]
        d = np.sqrt(((p[:, None, :] - v[None]) ** 2).sum(-1))
        m = min(k + 1, nv)
        part = np.argpartition(d, m - 1, axis=1)[:, :m]
        dp = np.take_along_axis(d, part, 1)
        order = np.lexsort((part, dp), axis=1)                     # by distance, then by vertex index
        part, dp = np.take_along_axis(part, order, 1), np.take_along_axis(dp, order, 1)
        if m > k:
            gap[s:s + chunk] = (dp[:, k] - dp[:, k - 1]) / np.maximum(dp[:, k], 1e-300)
        w = 1.0 / np.clip(dp[:, :k], 1e-4, 1.0)
        w /= w.sum(1, keepdims=True)
        out[s:s + chunk] = (ws[part[:, :k]] * w[:, :, None]).sum(1)
    return out, gap


def field(bmin, bmax, res, verts, vws, k, align_corners=False):
    """(field [nj,D,H,W] float64 before smoothing, gap [D H W])."""
    W, H, D = res
    b, gap = knn_blend(centres(bmin, bmax, res, align_corners), verts, vws, k)
    return np.ascontiguousarray(b.T).reshape(-1, D, H, W), gap


def smooth(f, times):
    """`times` Jacobi steps on f [nj,D,H,W] (any float type; computed in that type)."""
    f = f.copy()
    for _ in range(times):
        if min(f.shape[1:]) >= 3:
            c = f[:, 1:-1, 1:-1, 1:-1]
            mean = (f[:, 2:, 1:-1, 1:-1] + f[:, :-2, 1:-1, 1:-1] + f[:, 1:-1, 2:, 1:-1] + f[:, 1:-1, :-2, 1:-1] + f[:, 1:-1, 1:-1, 2:]
                    + f[:, 1:-1, 1:-1, :-2]) / 6.0
            new = f.copy()
            new[:, 1:-1, 1:-1, 1:-1] = (c - mean) * 0.7 + mean
            f = new
        f = f / f.sum(0, keepdims=True)
    return f


def mid_subsample():
    W, H, D = MID_GRID
    return np.arange(MID_STRIDE // 2, W * H * D, MID_STRIDE)


def bound(ref_err):
    return max(4.0 * float(ref_err), 1e-6)


def masked_error(ours, twin, gap):
    """(max |ours - twin| over the voxels kept, number excluded): voxels [.., n] along the last axis, those with gap < GAP_MIN left out
    only as far as EXCLUDE_CAP allows (the closest gaps first)."""
    err = np.abs(np.asarray(ours, np.float64) - twin).reshape(twin.shape[0], -1).max(0)
    gap = np.asarray(gap).reshape(-1)
    cand = np.nonzero(gap < GAP_MIN)[0]
    cap = int(EXCLUDE_CAP * gap.size)
    drop = cand[np.argsort(gap[cand])][:cap]
    keep = np.ones(gap.size, bool)
    keep[drop] = False
    return float(err[keep].max()), int(drop.size)
