"""Numpy restatement of the point-to-plane ICP alignment (selfreconcode_amd.align, csrc/icp.hip), written from the
stated semantics in float64: `_surfdist_ref.closest` / `sample` / `face_normals` for the geometry, plain loops for the Cholesky, numpy
for everything else.  It does not mirror the kernels' sample order or summation order; the tests compare through bounds.

The test shape: cube_sphere(n) bent out of every symmetry, v <- v (1 + 0.25 sin(3 v_x + 1) cos(2 v_y) + 0.2 v_z v_x), v <- v (1, 0.7,
0.45), rounded to float32; pred = R0^T (v - t0) / s0, so the transform that takes pred onto the shape is (s0, R0, t0)."""
import numpy as np

import _surfdist_ref as sr

PIVOT_MIN = 2. ** -20          # on the system scaled to a unit diagonal
COLUMN_MIN = 2. ** -46         # mean square of a column
TOL = 2. ** -23

CASES = {"rigid": (1., (1., 2., 3.), 12., (0.05, -0.08, 0.11)), "similarity": (1.08, (3., -1., 2.), 9., (-0.07, 0.04, 0.06))}


def shape(n):
    """(verts [V,3] float32, faces [F,3] int64) of the test shape."""
    from selfreconcode_amd.synthetic import cube_sphere
    v, f = [x.numpy() for x in cube_sphere(n)]
    v = v.astype(np.float64)
    v = v * (1. + 0.25 * np.sin(3. * v[:, 0] + 1.) * np.cos(2. * v[:, 1]) + 0.2 * v[:, 2] * v[:, 0])[:, None]
    v = v * np.float64([1., 0.7, 0.45])
    return v.astype(np.float32), f.astype(np.int64)


def exp_rotation(w):
    """exp of the rotation vector w [3], through the normalised half-angle quaternion."""
    w = np.asarray(w, np.float64)
    angle = np.sqrt((w * w).sum())
    q = np.float64([1., 0., 0., 0.])
    if angle > 0:
        q = np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) / angle * w])
        q = q / np.sqrt((q * q).sum())
    a, x, y, z = q
    return np.float64([[a * a + x * x - y * y - z * z, 2 * x * y - 2 * a * z, 2 * a * y + 2 * x * z],
                       [2 * a * z + 2 * x * y, a * a - x * x + y * y - z * z, 2 * y * z - 2 * a * x],
                       [2 * x * z - 2 * a * y, 2 * a * x + 2 * y * z, a * a - x * x - y * y + z * z]])


def case(name, n):
    """(pred, gt, (s0, R0, t0)) of a named case on shape(n): pred = (verts float32, faces), gt likewise."""
    s0, axis, deg, t0 = CASES[name]
    axis = np.float64(axis) / np.linalg.norm(axis)
    R0, t0 = exp_rotation(np.deg2rad(deg) * axis), np.float64(t0)
    v, f = shape(n)
    pred = ((v.astype(np.float64) - t0) @ R0 / s0).astype(np.float32)         # rows of R0^T (v - t0) / s0
    return (pred, f), (v, f), (s0, R0, t0)


def frame(verts):
    """(o [3], rho): centre and half diagonal of the box of the float32 vertices (rho = 1 for one point)."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    rho = 0.5 * np.sqrt(((hi - lo) ** 2).sum())
    return 0.5 * (lo + hi), rho if rho > 0 else 1.


def rows(q, c, n, o, rho):
    """[a | r] [K,8] of the pairs: q [K,3] transformed samples, c their closest points, n the unit normals of the closest faces."""
    x = (q - o) / rho
    return np.concatenate([np.cross(x, n), n, (n * x).sum(1)[:, None], ((n * (q - c)).sum(1) / rho)[:, None]], 1)


def scaled_system(G, count, scale):
    """(A [7,7], rhs [7], dsc [7], keep [7]) of the normal equations G = [a | r]^T [a | r] scaled to a unit diagonal: an unknown
    stays when it is asked for (sigma only with `scale`) and its column has a mean square above COLUMN_MIN."""
    diag = np.diag(G)[:7]
    keep = (np.arange(7) < (7 if scale else 6)) & (diag > count * COLUMN_MIN)
    dsc = np.where(keep, 1. / np.sqrt(np.where(keep, diag, 1.)), 0.)
    return G[:7, :7] * dsc[:, None] * dsc[None], -G[:7, 7] * dsc, dsc, keep


def solve(G, count, scale):
    """(xi [7], rank): Cholesky on the scaled system; an unknown whose pivot is below PIVOT_MIN is set to 0 and leaves the system."""
    A, rhs, dsc, keep = scaled_system(G, count, scale)
    keep = keep.copy()
    L, y, z = np.zeros((7, 7)), np.zeros(7), np.zeros(7)
    for j in range(7):
        if not keep[j]:
            continue
        p = A[j, j] - (L[j, :j] ** 2).sum()
        if not p >= PIVOT_MIN:
            keep[j] = False
            L[j, :j] = 0.
            continue
        L[j, j] = np.sqrt(p)
        for i in range(j + 1, 7):
            if keep[i]:
                L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    for j in range(7):
        if keep[j]:
            y[j] = (rhs[j] - (L[j, :j] * y[:j]).sum()) / L[j, j]
    for j in range(6, -1, -1):
        if keep[j]:
            z[j] = (y[j] - (L[j + 1:, j] * z[j + 1:] * keep[j + 1:]).sum()) / L[j, j]
    return np.where(keep, z * dsc, 0.), int(keep.sum())


def solve_lstsq(G, count, scale):
    """xi of the same scaled system by numpy.linalg.lstsq on the unknowns scaled_system keeps (a full-rank system: the same answer
    up to the float64 noise of that system)."""
    A, rhs, dsc, keep = scaled_system(G, count, scale)
    k = np.flatnonzero(keep)
    xi = np.zeros(7)
    xi[k] = np.linalg.lstsq(A[np.ix_(k, k)], rhs[k], rcond=None)[0] * dsc[k]
    return xi


def update(M, t, xi, o, rho):
    """(M, t) after the update xi = (omega, tau, sigma)."""
    R, sd = exp_rotation(xi[:3]), 1. + xi[6]
    return sd * (R @ M), o + sd * (R @ (t - o)) + rho * xi[3:6]


def centroid_init(p, g, scale):
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    cp, cg = p.mean(0), g.mean(0)
    s = np.sqrt(((g - cg) ** 2).sum(1).mean() / ((p - cp) ** 2).sum(1).mean()) if scale else 1.
    return s * np.eye(3), cg - s * cp


def samples_of(mesh, n, seed):
    """[n,3] float32 surface samples, as the sampler rounds them."""
    return sr.sample(sr.face_areas_cum(mesh[0], mesh[1]), mesh[0], mesh[1], n, seed)[0].astype(np.float32)


def icp(pred, gt, samples, seed=0, iters=30, scale=False, max_dist=np.inf, tol=TOL, init="centroid", dtype=np.float64, points=None):
    """The alignment of pred onto gt as a dict: matrix [4,4], iterations, converged, rank, history [iters,6].  `dtype` is the number
    format of the closest-point search alone (float32: the noise floor of the kernels' search); `points` replaces the samples."""
    p = (samples_of(pred, samples, seed) if points is None else np.asarray(points, np.float32)).astype(np.float64)
    if isinstance(init, str) and init == "centroid":
        M, t = centroid_init(p, samples_of(gt, len(p), seed + 1), scale)
    elif isinstance(init, str):
        M, t = np.eye(3), np.zeros(3)
    else:
        M, t = np.float64(init)[:3, :3].copy(), np.float64(init)[:3, 3].copy()
    o, rho = frame(gt[0])
    normals = sr.face_normals(gt[0], gt[1])
    history, done, live = np.zeros((iters, 6)), False, 0
    for it in range(iters):
        if done:
            history[it] = history[it - 1]
            history[it, 5] = 1.
            continue
        q = (p @ M.T + t).astype(np.float32)
        ok = np.isfinite(q).all(1)
        d, f, c = sr.closest(q[ok], gt[0], gt[1], dtype)
        d, c = d.astype(np.float64), c.astype(np.float64)
        near = d <= max_dist
        W = rows(q[ok][near].astype(np.float64), c[near], normals[f[near]], o, rho)
        count = float(near.sum())
        xi, rank = solve(W.T @ W, count, scale)
        M, t = update(M, t, xi, o, rho)
        done, live = bool(np.abs(xi).max() < tol), it + 1
        history[it] = [count, np.sqrt((d[near] ** 2).sum() / count) if count else 0., np.abs(xi).max(), rank, np.sqrt((M * M).sum() / 3.), done]
    matrix = np.eye(4)
    matrix[:3, :3], matrix[:3, 3] = M, t
    return {"matrix": matrix, "iterations": live, "converged": done, "rank": int(history[live - 1, 3]), "history": history}


def truth_matrix(answer):
    s0, R0, t0 = answer
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = s0 * R0, t0
    return m


def flat_pair(offset=0.05):
    """A flat square of 2 x 2 cells (8 triangles) in the plane z = 0, and a copy lifted by `offset` along its normal."""
    g = np.float32([[i, j, 0.] for j in range(3) for i in range(3)]) * np.float32(0.5)
    f = []
    for j in range(2):
        for i in range(2):
            a = j * 3 + i
            f += [[a, a + 1, a + 4], [a, a + 4, a + 3]]
    f = np.int64(f)
    return (g + np.float32([0., 0., offset]), f), (g, f)
