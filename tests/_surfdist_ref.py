"""Numpy restatement of the surface-distance evaluation (selfreconcode_amd.evaluate / surfdist_ops), written from the
stated semantics and not from the kernels: no grid, no rings.  `closest` in float64 is the truth and in float32 the noise floor of the
number format.

Distance rule (one triangle): the orthogonal projection if the triangle has a positive area and the projection lies inside it,
otherwise the nearest of the three edges as clamped segments; a zero-length edge is its end point.  The distance is |p - q|.

`closest` looks at every face (prune=False) or only at the faces that can hold the minimum (prune=True: a face whose centroid is
farther than the nearest centroid by more than the largest face radius cannot; the centroid is a point of the face).  The selection is
the same whatever `dtype` is, so both dtypes evaluate the same candidates."""
import numpy as np

from selfreconcode_amd.synthetic import _splitmix


def _dot(a, b):
    return (a * b).sum(-1)


def tri_eval(p, a, b, c):
    """(d2 [N], q [N,3]) of points p [N,3] against triangles (a, b, c) [N,3] each, in the arrays' dtype."""
    dt = p.dtype
    zero, one = dt.type(0), dt.type(1)
    best = np.full(p.shape[0], np.inf, dt)
    q = np.zeros_like(p)
    for s, e in ((a, b), (b, c), (c, a)):
        d = e - s
        dd = _dot(d, d)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(dd > 0, _dot(p - s, d) / np.where(dd > 0, dd, one), zero)
        t = np.clip(t, zero, one).astype(dt)
        cand = s + t[:, None] * d
        r = p - cand
        d2 = _dot(r, r)
        take = d2 < best
        best = np.where(take, d2, best)
        q = np.where(take[:, None], cand, q)
    u, v, w = b - a, c - a, p - a
    n = np.cross(u, v)
    nn = _dot(n, n)
    safe = np.where(nn > 0, nn, one)
    gamma = _dot(np.cross(u, w), n) / safe
    beta = _dot(np.cross(w, v), n) / safe
    inside = (nn > 0) & (beta >= 0) & (gamma >= 0) & (one - beta - gamma >= 0)
    proj = a + beta[:, None] * u + gamma[:, None] * v
    r = p - proj
    best = np.where(inside, _dot(r, r), best)
    q = np.where(inside[:, None], proj, q)
    return best.astype(dt), q.astype(dt)


def _candidates(p64, tri64, chunk):
    """(point index, face index) of the pairs worth evaluating, sorted by point and then by face.  The squared centroid distances come
    from a float32 matrix product: that only selects, and its error (below 2e-6 scale^2, so below 1.5e-3 scale in a distance) is in
    the margin."""
    cen = tri64.mean(1)
    rad = float(np.sqrt(((tri64 - cen[:, None]) ** 2).sum(-1)).max())
    scale = max(float(np.abs(p64).max(initial=0.)), float(np.abs(tri64).max(initial=0.)), 1e-30)
    c32, p32 = cen.astype(np.float32), p64.astype(np.float32)
    pi, fi, cc = [], [], (c32 * c32).sum(1)
    for s in range(0, len(p32), chunk):
        part = p32[s:s + chunk]
        d2 = part @ (-2. * c32.T)
        d2 += (part * part).sum(1)[:, None]
        d2 += cc[None]
        reach = np.sqrt(np.maximum(d2.min(1), 0.)).astype(np.float64) + rad + 4e-3 * scale
        i, f = np.nonzero(d2 <= (reach * reach).astype(np.float32)[:, None] * np.float32(1.0001))
        pi.append(i + s); fi.append(f)
    return np.concatenate(pi), np.concatenate(fi)


def closest(points, verts, faces, dtype=np.float64, prune=True, chunk=None):
    """(dist [P], face [P] (the lowest index among equal squared distances), closest [P,3]) in `dtype`."""
    p64 = np.asarray(points, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tri64 = np.asarray(verts, np.float32).astype(np.float64)[f]
    P, F = len(p64), len(f)
    chunk = chunk or max(1, 2_000_000 // max(F, 1))
    if prune:
        pi, fi = _candidates(p64, tri64, chunk)
    else:
        pi, fi = np.repeat(np.arange(P), F), np.tile(np.arange(F), P)
    d2 = np.empty(len(pi), dtype); q = np.empty((len(pi), 3), dtype)
    p, tri = p64.astype(dtype), tri64.astype(dtype)
    step = 1_000_000
    for s in range(0, len(pi), step):
        a = slice(s, s + step)
        d2[a], q[a] = tri_eval(p[pi[a]], tri[fi[a], 0], tri[fi[a], 1], tri[fi[a], 2])
    starts = np.searchsorted(pi, np.arange(P))
    mins = np.minimum.reduceat(d2, starts)
    hit = np.flatnonzero(d2 == mins[pi])
    _, first = np.unique(pi[hit], return_index=True)
    sel = hit[first]
    return np.sqrt(d2[sel]), fi[sel], q[sel]


def face_distance(points, verts, faces, face):
    """float64 distance from point i to face[i] alone."""
    p = np.asarray(points, np.float64)
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)[np.asarray(face, np.int64)]]
    return np.sqrt(tri_eval(p, tri[:, 0], tri[:, 1], tri[:, 2])[0])


def face_areas_cum(verts, faces):
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    return np.cumsum(0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1))


def face_normals(verts, faces):
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(length > 0, n / np.where(length > 0, length, 1.), 0.)


def sample(cum_area, verts, faces, n, seed):
    """(points [n,3] float64, face [n], normals [n,3] float64): sample i at r = (i + xi) / n A on the first face with cum_area > r (the
    first that reaches A when r rounds up to A), barycentrics (1 - sqrt u, sqrt u (1 - v), sqrt u v), (xi, u, v) = (splitmix(3 i + {0,
    1, 2}, seed) >> 11) 2^-53."""
    cum = np.asarray(cum_area, np.float64)
    A = cum[-1]
    i = np.arange(n, dtype=np.uint64)
    xi, u, v = ((_splitmix(np.uint64(3) * i + np.uint64(k), seed) >> np.uint64(11)).astype(np.float64) * 2. ** -53 for k in range(3))
    r = (np.arange(n, dtype=np.float64) + xi) / float(n) * A
    face = np.searchsorted(cum, r, side="right")
    top = ~(r < A)
    face[top] = np.searchsorted(cum, A, side="left")
    tri = np.asarray(verts, np.float32).astype(np.float64)[np.asarray(faces, np.int64)[face]]
    su = np.sqrt(u)
    pts = (1. - su)[:, None] * tri[:, 0] + (su * (1. - v))[:, None] * tri[:, 1] + (su * v)[:, None] * tri[:, 2]
    return pts, face, face_normals(verts, faces)[face]


def metrics(pred, gt, pred_samples, gt_samples, taus=()):
    """The metrics of surface_metrics from given samples: pred / gt = (verts, faces), *_samples = (points [n,3], normals [n,3])."""
    out, dots, dist = {}, [], {}
    for name, (pts, nrm), mesh in (("pred_to_gt", pred_samples, gt), ("gt_to_pred", gt_samples, pred)):
        d, f, _ = closest(pts, mesh[0], mesh[1])
        dist[name] = d
        out[name] = {"mean": float(d.mean()), "rms": float(np.sqrt((d * d).mean())), "max": float(d.max())}
        dots.append(float((np.asarray(nrm, np.float64) * face_normals(mesh[0], mesh[1])[f]).sum(1).mean()))
    out["chamfer"] = 0.5 * (out["pred_to_gt"]["mean"] + out["gt_to_pred"]["mean"])
    out["p2s"] = out["gt_to_pred"]["mean"]
    out["normal_consistency"] = 0.5 * (dots[0] + dots[1])
    for t in taus:
        p, r = float((dist["pred_to_gt"] < t).mean()), float((dist["gt_to_pred"] < t).mean())
        out[f"fscore@{float(t):g}"] = 2. * p * r / (p + r) if p + r > 0 else 0.
    return out
