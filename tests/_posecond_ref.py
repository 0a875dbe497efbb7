"""Float64 numpy restatements of the pose conditioning (selfreconcode_amd/posecond_ops.py): the pose feature, the
brute-force neighbour search, the code blend and the sigma calibration.  Nothing here is shared with the code under test."""
import numpy as np

JOINTS, FEATS = 23, 207


def rodrigues(t):
    """[..., 3] axis-angle -> [..., 3, 3] through the half-angle quaternion with +1e-8 inside the norm, as the body model does it."""
    t = np.asarray(t, np.float64)
    angle = np.sqrt(((t + 1e-8) ** 2).sum(-1, keepdims=True))
    n = t / angle
    half = angle * 0.5
    q = np.concatenate([np.cos(half), np.sin(half) * n], -1)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                  2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                  2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], -1)
    return R.reshape(t.shape[:-1] + (3, 3))


def features(theta, joint_weights=None):
    """[N, 207]: (R_j - I) sqrt(w_j) for joints 1 .. 23 of theta [N,24,3] (or [N,72]), row major within a joint."""
    theta = np.asarray(theta, np.float64).reshape(-1, 24, 3)
    f = rodrigues(theta[:, 1:]) - np.eye(3)
    if joint_weights is not None:
        f = f * np.sqrt(np.asarray(joint_weights, np.float64)).reshape(1, JOINTS, 1, 1)
    return f.reshape(theta.shape[0], FEATS)


def distances(featq, feat):
    """[Q, N] squared distances of feature rows."""
    featq, feat = np.asarray(featq, np.float64), np.asarray(feat, np.float64)
    return ((featq[:, None, :] - feat[None, :, :]) ** 2).sum(-1)


def allowed(Q, N, query_frames=None, exclude=-1):
    """[Q, N] bool: frame n is a candidate of query q."""
    ok = np.ones((Q, N), bool)
    if query_frames is not None and exclude >= 0:
        ok &= np.abs(np.arange(N)[None, :] - np.asarray(query_frames, np.int64)[:, None]) > exclude
    return ok


def neighbors(D, K, query_frames=None, exclude=-1):
    """(idx [Q,K], d2 [Q,K]) from distances D [Q,N]: the K smallest finite allowed ones in ascending (d2, n); -1 / inf where none."""
    D = np.array(D, np.float64)
    Q, N = D.shape
    D[~allowed(Q, N, query_frames, exclude) | ~np.isfinite(D)] = np.inf
    order = np.argsort(D, axis=1, kind='stable')[:, :K]
    d2 = np.take_along_axis(D, order, 1)
    idx = np.where(np.isinf(d2), -1, order)
    if N < K:
        idx = np.concatenate([idx, np.full((Q, K - N), -1)], 1)
        d2 = np.concatenate([d2, np.full((Q, K - N), np.inf)], 1)
    return idx, d2


def blend(idx, d2, codes, sigma2):
    """(out [Q,L], weights [Q,K]): weights exp(-(d2_k - d2_0) / (2 sigma2)) over idx >= 0, normalised; zeros for a row without one."""
    idx, d2, codes = np.asarray(idx), np.asarray(d2, np.float64), np.asarray(codes, np.float64)
    valid = idx >= 0
    first = np.argmax(valid, axis=1)
    base = np.where(valid.any(1), d2[np.arange(idx.shape[0]), first], 0.)
    with np.errstate(invalid='ignore', over='ignore'):
        w = np.where(valid, np.exp(-(np.where(valid, d2, 0.) - base[:, None]) / (2. * sigma2)), 0.)
    s = w.sum(1, keepdims=True)
    w = np.where(s > 0, w / np.where(s > 0, s, 1.), 0.)
    return (w[:, :, None] * codes[np.where(valid, idx, 0)]).sum(1), w


def calibrate(d2_nearest):
    """The lower median of the finite entries of d2_nearest [N] (each frame's distance to its nearest allowed frame); None for none."""
    d = np.sort(np.asarray(d2_nearest, np.float64)[np.isfinite(d2_nearest)])
    return None if d.size == 0 else float(d[(d.size - 1) // 2])
